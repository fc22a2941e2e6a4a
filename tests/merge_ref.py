"""The map-point merge of loop closure restated literally (include/airfe.h "Map-point merge"; airslam_amd/csrc/merge_core.h): the reference's std::map /
std::set as Python dicts and sorted sets, the group-building loop of MapRefiner::MergeMappoints (src/map_refiner.cc:618-651) as written, MergeMappointGroup
(:668-713) over observer dicts derived from the id table; the epipolar gate computed independently as numpy.linalg.inv(K.T) @ tx @ R @ K.  Also the hand
cases and seeded tables the CPU and GPU tests share, and the host statement compiled with the host compiler."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
F_, CAP, P_ = 80, 64, 2048                  # the database of every case: max_frames, cap, max_points
CAM = (458.654, 457.296, 367.215, 248.375)
I3 = np.eye(3)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------
def epipolar_er(cam, R, t, p1, p2):
    """er of check_epipolar (:338-352), numpy's own way"""
    fx, fy, cx, cy = cam
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])
    with np.errstate(all="ignore"):
        Fm = np.linalg.inv(K.T) @ tx @ np.asarray(R, np.float64).reshape(3, 3) @ K
        el = Fm @ np.array([float(p1[0]), float(p1[1]), 1.0])
        s = np.linalg.norm(el[:2])
        return float(np.float64(np.array([float(p2[0]), float(p2[1]), 1.0]) @ el) / np.float64(s))


def entries(case):
    """step 1 over a loop case -> [(q, e, kind, fq, qi, bf, ci, er)] with kind in dead / outlier / epipolar / live; er only where the gate was computed"""
    ids, xyz, xy, n, size, L = case["ids"], case["xyz"], case["xy"], case["n"], case["size"], case["loop"]
    cap = ids.shape[1]
    rows = lambda f: min(max(int(n[f]), 0), cap)  # noqa: E731
    out = []
    for q in range(len(L["qframe"])):
        if L["stage"][q] != 0:
            continue
        fq, bf = int(L["qframe"][q]), int(L["loop"][q])
        for e in range(min(max(int(L["nmatch"][q]), 0), L["mcap"])):
            qi, ci = int(L["idx"][q, e, 0]), int(L["idx"][q, e, 1])
            kind, er = "live", None
            if not (0 <= fq < size and 0 <= bf < size) or qi < 0 or ci < 0 or qi >= rows(fq) or ci >= rows(bf) or not 0 <= ids[bf, ci] < case["P"]:
                kind = "dead"
            elif not np.isnan(xyz[bf, ci, 0]):
                if L["mask"][q, e] == 0:
                    kind = "outlier"
            else:
                er = epipolar_er(L["cam"], L["Rlq"][q], L["tlq"][q], xy[fq, qi], xy[bf, ci])
                if not er < 10:
                    kind = "epipolar"
            out.append((q, e, kind, fq, qi, bf, ci, er))
    return out


def merge(case):
    """-> (ids, xyz, map, info) after the call"""
    before_ids, before_xyz, n, size, P = case["ids"], case["xyz"], case["n"], case["size"], case["P"]
    cap = before_ids.shape[1]
    rows = lambda f: min(max(int(n[f]), 0), cap)  # noqa: E731
    valid = lambda m: 0 <= m < P  # noqa: E731
    info = [0] * 8
    merged = {}                              # std::map<mappoint on the query frame, std::set<matched mappoint>>
    adopt = {}                               # (f, i) -> the B of every live entry that finds no mappoint there
    if case.get("loop") is not None:
        for q, e, kind, fq, qi, bf, ci, er in entries(case):
            info[{"live": 0, "outlier": 1, "epipolar": 2}.get(kind, 0)] += kind != "dead"
            if kind != "live":
                continue
            A, B = int(before_ids[fq, qi]), int(before_ids[bf, ci])
            if valid(A):
                merged.setdefault(A, set()).add(B)
            else:
                adopt.setdefault((fq, qi), set()).add(B)
    else:
        for A, B in np.asarray(case["pairs"], np.int64).reshape(-1, 2).tolist():
            if valid(A) and valid(B):
                info[0] += 1
                merged.setdefault(A, set()).add(B)
            else:
                info[1] += 1
    src = {}                                 # the first triangulated row of every id, on the tables as they were
    for f in range(size):
        for i in range(rows(f)):
            m = int(before_ids[f, i])
            if valid(m) and not np.isnan(before_xyz[f, i, 0]):
                src.setdefault(m, (f, i))
    pos = lambda m: before_xyz[src[m]] if m in src else np.full(3, np.nan)  # noqa: E731
    ids, xyz = before_ids.copy(), before_xyz.copy()
    for (f, i), Bs in adopt.items():         # :452-457, the smallest B for a row several entries adopt
        b = min(Bs)
        ids[f, i], xyz[f, i] = b, pos(b)
        merged.setdefault(b, set()).update(Bs)
        info[3] += 1
    # ---- MergeMappoints (:608-651)
    for k in merged:
        merged[k].add(k)
    mpt_id_to_group_id, mappoint_groups, new_group_id = {}, {}, 0
    for k in sorted(merged):
        found_groups = sorted({mpt_id_to_group_id[m] for m in merged[k] if m in mpt_id_to_group_id})
        if len(found_groups) == 0:
            best_group_id = new_group_id
            new_group_id += 1
        elif len(found_groups) == 1:
            best_group_id = found_groups[0]
        else:
            best_group_id = found_groups[0]
            for group_id in found_groups:
                if group_id == best_group_id:
                    continue
                for m in sorted(mappoint_groups[group_id]):
                    mpt_id_to_group_id[m] = best_group_id
                    mappoint_groups.setdefault(best_group_id, set()).add(m)
                del mappoint_groups[group_id]
        for m in sorted(merged[k]):
            mpt_id_to_group_id[m] = best_group_id
            mappoint_groups.setdefault(best_group_id, set()).add(m)
    # ---- the observers the id table implies after adoption: per id {frame: first row} and every row
    grouped = {m for g in mappoint_groups.values() if len(g) >= 2 for m in g}
    observers, held = {m: {} for m in grouped}, {m: [] for m in grouped}
    for f in range(size):
        for i in range(rows(f)):
            m = int(ids[f, i])
            if m in grouped:
                observers[m].setdefault(f, i)
                held[m].append((f, i))
    # ---- MergeMappointGroup (:668-713)
    mp = np.arange(P, dtype=np.int32)
    for gid in sorted(mappoint_groups):
        group = sorted(mappoint_groups[gid])
        if len(group) < 2:
            continue
        info[4] += 1
        info[5] += len(group) - 1
        best = next((m for m in group if m in src), group[0])
        obversers_of_best, given = dict(observers[best]), set()
        for m in group:
            if m == best:
                continue
            for f in sorted(observers[m]):
                if f not in obversers_of_best:
                    obversers_of_best[f] = observers[m][f]
                    given.add((f, observers[m][f]))
        for m in group:
            mp[m] = best
            if m == best:
                continue
            for at in held[m]:               # SetBad + erase: what still points at m is a bad pointer, -1 in the table
                if at in given:
                    ids[at], xyz[at] = best, pos(best)
                    info[6] += 1
                else:
                    ids[at], xyz[at] = -1, np.nan
                    info[7] += 1
    return ids, xyz, mp, info


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------------
class Scene:
    """a database's tables with nothing in them: size frames of n rows, keypoints anywhere in the image"""

    def __init__(self, seed=0, size=72, n=48):
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.ids = np.full((F_, CAP), -1, np.int32)
        self.xyz = np.full((F_, CAP, 3), np.nan)
        self.xy = rng.uniform(5.0, 700.0, (F_, CAP, 2)).astype(np.float32)
        self.n = np.full(F_, n, np.int32)
        self.size = size
        self.q = []

    def put(self, f, i, m, tri=True):
        self.ids[f, i] = m
        self.xyz[f, i] = self.rng.uniform(-5, 5, 3) if tri else np.nan
        return self

    def query(self, fq, bf, ent, stage=0, R=I3, t=(0.3, 0.05, -0.1), nmatch=None):
        """ent: [(qi, ci, mask)]"""
        self.q.append(dict(fq=fq, bf=bf, ent=list(ent), stage=stage, R=np.asarray(R, np.float64), t=np.asarray(t, np.float64), nmatch=nmatch))
        return self

    def aim(self, fq, qi, bf, ci, er, R=I3, t=(0.3, 0.05, -0.1)):
        """move keypoint (bf, ci) so that the epipolar gate of (fq, qi) -> (bf, ci) gives about `er`"""
        fx, fy, cx, cy = CAM
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])
        el = np.linalg.inv(K.T) @ tx @ np.asarray(R, np.float64) @ K @ np.array([*self.xy[fq, qi].astype(np.float64), 1.0])
        x2 = float(self.xy[bf, ci, 0])
        self.xy[bf, ci, 1] = np.float32((er * np.linalg.norm(el[:2]) - x2 * el[0] - el[2]) / el[1])
        return self

    def case(self, name, pairs=None, mcap=32):
        c = dict(name=name, ids=self.ids, xyz=self.xyz, xy=self.xy, n=self.n, size=self.size, P=P_, loop=None, pairs=None)
        if pairs is not None:
            c["pairs"] = np.asarray(pairs, np.int32).reshape(-1, 2)
            return c
        Q = len(self.q)
        L = dict(qframe=np.zeros(Q, np.int32), stage=np.zeros(Q, np.int32), loop=np.zeros(Q, np.int32), Rlq=np.zeros((Q, 9)), tlq=np.zeros((Q, 3)),
                 mask=np.full((Q, mcap), 7, np.uint8), idx=np.full((Q, mcap, 2), -9, np.int32), nmatch=np.zeros(Q, np.int32), mcap=mcap, cam=CAM)
        for k, q in enumerate(self.q):
            L["qframe"][k], L["stage"][k], L["loop"][k], L["Rlq"][k], L["tlq"][k] = q["fq"], q["stage"], q["bf"], q["R"].reshape(9), q["t"]
            for e, (qi, ci, m) in enumerate(q["ent"]):
                L["idx"][k, e], L["mask"][k, e] = (qi, ci), m
            L["nmatch"][k] = len(q["ent"]) if q["nmatch"] is None else q["nmatch"]
        c["loop"] = L
        return c


def _chain(order):
    """ids 100 .. 1099, id m at frame m % 70 row (m // 70): a 1000-id chain linked in `order`"""
    s = Scene(3)
    for k in range(1000):
        s.put(k % 70, k // 70, 100 + k, tri=(k % 7 == 3))
    links = [(100 + k, 101 + k) for k in range(999)]
    if order == "descending":
        links = [(b, a) for a, b in links[::-1]]
    elif order == "shuffled":
        rng = np.random.default_rng(5)
        links = [links[j] if rng.random() < 0.5 else links[j][::-1] for j in rng.permutation(999)]
    return s.case("chain1000_" + order, pairs=links)


def hand_cases():
    out = []
    # ---- the pair form
    s = Scene(1).put(0, 0, 10).put(1, 3, 11).put(2, 1, 10)
    out.append(s.case("one_pair", pairs=[(11, 10)]))
    s = Scene(2)
    for k, m in enumerate((20, 21, 22, 23)):
        s.put(k, k, m, tri=(m == 22)).put(10 + k, 2, m, tri=False)
    out.append(s.case("best_is_not_the_smallest", pairs=[(20, 21), (21, 22), (22, 23)]))
    s = Scene(4)
    for k in range(301):
        s.put(k % 70, k // 70, 500 + k, tri=(k % 3 == 1))
    out.append(s.case("star300", pairs=[(500 + k, 500) if k % 2 else (500, 500 + k) for k in range(1, 301)]))
    out += [_chain(o) for o in ("ascending", "descending", "shuffled")]
    s = Scene(6).put(0, 0, 30, tri=False).put(1, 0, 31, tri=False).put(1, 5, 32, tri=False).put(2, 2, 32, tri=False)
    out.append(s.case("no_triangulated_member", pairs=[(31, 30), (32, 31)]))
    s = Scene(7).put(0, 1, 40).put(0, 2, 41).put(0, 3, 42, tri=False).put(1, 1, 41).put(1, 4, 42)
    out.append(s.case("frame_holds_best_and_members", pairs=[(40, 41), (42, 41)]))
    s = Scene(8).put(0, 0, 50).put(1, 7, 52).put(1, 2, 51).put(1, 9, 52).put(2, 3, 51, tri=False)
    out.append(s.case("frame_holds_two_non_best", pairs=[(52, 50), (51, 50)]))
    s = Scene(9).put(0, 0, 60).put(1, 5, 61).put(1, 2, 61, tri=False).put(1, 8, 61).put(2, 1, 60).put(2, 6, 60, tri=False).put(2, 7, 61)
    out.append(s.case("one_id_at_two_rows", pairs=[(61, 60)]))
    s = Scene(10).put(0, 0, 70).put(1, 0, 71).put(2, 0, 72)
    out.append(s.case("ids_out_of_range", pairs=[(70, P_), (-1, 71), (71, 70), (2 ** 31 - 1, -2 ** 31), (72, 72), (P_ - 1, P_ - 1)]))
    out.append(Scene(11).put(0, 0, 80).case("no_pairs", pairs=[]))
    # ---- the loop form
    s = Scene(20)                            # a chain a-b, b-c, c-d over different queries
    for k, m in enumerate((90, 91, 92, 93)):
        s.put(10 + k, 1, m).put(20 + k, 2, m)
    s.put(11, 3, 90, tri=False).put(21, 4, 91, tri=False).put(12, 5, 93, tri=False)
    for order in ("fwd", "rev"):
        t = Scene(20)
        t.ids, t.xyz, t.xy = s.ids, s.xyz, s.xy
        qs = [(10, 21, [(1, 2, 1)]), (11, 22, [(1, 2, 1)]), (12, 23, [(1, 2, 1)])]
        for fq, bf, ent in (qs if order == "fwd" else qs[::-1]):
            t.query(fq, bf, ent)
        out.append(t.case("chain_over_queries_" + order))
    s = Scene(21).put(30, 0, 200).put(30, 1, 201, tri=False).put(30, 2, 202).put(31, 0, 203, tri=False)
    s.query(40, 30, [(0, 0, 1), (1, 1, 1), (2, 2, 0)]).aim(40, 1, 30, 1, 4.0)
    out.append(s.case("adoption"))
    s = Scene(22).put(30, 0, 210).put(30, 1, 205).put(31, 0, 207, tri=False).put(32, 4, 205, tri=False).put(33, 4, 207)
    s.query(41, 30, [(5, 0, 1), (5, 1, 1)]).query(41, 31, [(5, 0, 1)]).aim(41, 5, 31, 0, -3.0)
    out.append(s.case("two_entries_adopt_one_row"))
    s = Scene(23).put(30, 0, 220).put(30, 1, 221).put(42, 0, 222).put(42, 1, 223)
    s.query(42, 30, [(0, 0, 0), (1, 1, 1), (0, 1, 0)])
    out.append(s.case("mask_zero_entries"))
    s = Scene(24)
    for k in range(3):
        s.put(30, k, 230 + k, tri=False).put(43, k, 240 + k)
    R = np.array([[0.9998, -0.02, 0.0], [0.02, 0.9998, 0.0], [0.0, 0.0, 1.0]])
    s.query(43, 30, [(0, 0, 0), (1, 1, 0)], R=R, t=(0.2, -0.1, 0.05)).aim(43, 0, 30, 0, 6.5, R, (0.2, -0.1, 0.05)).aim(43, 1, 30, 1, 14.0, R, (0.2, -0.1, 0.05))
    s.query(43, 30, [(2, 2, 1)], t=(0.0, 0.0, 0.0))                 # tlq = 0: F = 0, er = 0 / 0 fails
    out.append(s.case("epipolar_pass_fail_nan"))
    s = Scene(25).put(30, 0, 250).put(44, 0, 251).put(45, 0, 252).put(46, 0, 253).put(47, 0, 254).put(48, 0, 255).put(49, 0, 256)
    for k, st in enumerate((1, 2, 3, 4, 5, 0, -1)):
        s.query(44 + k, 30, [(0, 0, 1)], stage=st)
    out.append(s.case("stages_1_to_5"))
    s = Scene(26, size=60).put(30, 0, 260).put(30, 50, 261).put(44, 0, 262).put(44, 50, 263).put(65, 0, 264).put(30, 1, P_ + 5).put(30, 2, 265).put(44, 2, -7)
    s.query(44, -1, [(0, 0, 1)]).query(44, 60, [(0, 0, 1)]).query(65, 30, [(0, 0, 1)]).query(-3, 30, [(0, 0, 1)])
    s.query(44, 30, [(0, 50, 1), (50, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 1, 1), (0, 48, 1), (2, 2, 1)])
    s.query(44, 30, [(0, 0, 1)] * 3, nmatch=-2).query(44, 30, [(0, 0, 1)] * 3, nmatch=1000)
    out.append(s.case("dead_entries", mcap=8))
    out.append(Scene(27).put(0, 0, 270).case("no_queries"))
    s = Scene(28).put(30, 0, 280).put(44, 0, 281)
    s.query(44, 30, [(0, 0, 0)]).query(44, 31, [(0, 0, 1)], stage=3)
    out.append(s.case("no_live_entry"))
    return out


def seeded_case(seed, Q=40, mcap=48, ids_in_play=400):
    """a busy table: ~ids_in_play ids over 72 frames, 60 % of the rows with a position, queries that repeat frames and rows, hostile entries"""
    s = Scene(100 + seed)
    rng = s.rng
    s.n[:] = rng.integers(0, CAP + 1, F_)
    s.n[rng.integers(0, 72, 4)] = 0
    s.ids[:] = rng.integers(0, ids_in_play, (F_, CAP))
    s.ids[rng.random((F_, CAP)) < 0.35] = -1
    bad = rng.random((F_, CAP)) < 0.01
    s.ids[bad] = rng.choice(np.array([P_, -2, 2 ** 31 - 1, -2 ** 31], np.int64), int(bad.sum())).astype(np.int32)
    tri = rng.random(ids_in_play) < 0.6                              # an id is triangulated in most of its rows or in none
    has = (s.ids >= 0) & (s.ids < ids_in_play) & tri[np.clip(s.ids, 0, ids_in_play - 1)] & (rng.random((F_, CAP)) < 0.8)
    s.xyz[has] = rng.uniform(-5, 5, (int(has.sum()), 3))
    for k in range(Q):
        fq, bf = int(rng.integers(40, 74)), int(rng.integers(0, 40))
        nq, nb = max(int(s.n[fq]), 1), max(int(s.n[bf]), 1)          # most entries inside the counts, one in eight anywhere
        ent = [(int(rng.integers(0, nq)), int(rng.integers(0, nb))) if rng.random() < 0.875 else (int(rng.integers(-1, CAP + 1)), int(rng.integers(-1, CAP + 1)))
               for _ in range(int(rng.integers(0, mcap + 1)))]
        ent = [(qi, ci, int(rng.random() < 0.7) * int(rng.integers(1, 255))) for qi, ci in ent]
        ang = rng.uniform(-0.1, 0.1)
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
        s.query(fq if rng.random() < 0.9 else int(rng.integers(-2, 90)), bf if rng.random() < 0.9 else -1, ent, stage=int(rng.random() < 0.15) * int(rng.integers(1, 6)),
                R=R, t=rng.uniform(-0.5, 0.5, 3))
    return s.case(f"seeded{seed}", mcap=mcap)


def permuted(case, seed):
    """the same loop case with the query list and every list's entries permuted"""
    rng = np.random.default_rng(seed)
    L = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case["loop"].items()}
    for q in range(len(L["qframe"])):
        m = min(max(int(L["nmatch"][q]), 0), L["mcap"])
        p = rng.permutation(m)
        L["idx"][q, :m], L["mask"][q, :m] = L["idx"][q, :m][p], L["mask"][q, :m][p]
    p = rng.permutation(len(L["qframe"]))
    for k in ("qframe", "stage", "loop", "Rlq", "tlq", "mask", "idx", "nmatch"):
        L[k] = np.ascontiguousarray(L[k][p])
    return dict(case, loop=L)


def poisoned(case):
    """the same case with the tables' rows beyond n[f] and frames beyond size holding anything"""
    ids, xyz, xy = case["ids"].copy(), case["xyz"].copy(), case["xy"].copy()
    junk = np.array([7, 2 ** 31 - 1, -2 ** 31, 0, P_ - 1, P_], np.int64).astype(np.int32)
    cap = ids.shape[1]
    for f in range(ids.shape[0]):
        k = min(max(int(case["n"][f]), 0), cap) if f < case["size"] else 0
        ids[f, k:] = junk[(np.arange(cap - k) + f) % len(junk)]
        xyz[f, k:] = 3.25 + f
        xy[f, k:] = -1e30
    return dict(case, ids=ids, xyz=xyz, xy=xy)


# ---- the host statement ---------------------------------------------------------------------------------------------------------------------------------
SHIM = r'''
#include "merge_core.h"
static MergeTables tables(int32_t* point_id, double* xyz, const float* feat, const int* n, int size, int cap, int feat_dim, int max_points) {
  MergeTables t;
  t.point_id = point_id; t.xyz = xyz; t.feat = feat; t.n = n; t.size = size; t.cap = cap; t.feat_dim = feat_dim; t.max_points = max_points;
  return t;
}
extern "C" void core_loop(int32_t* point_id, double* xyz, const float* feat, const int* n, int size, int max_frames, int cap, int feat_dim, int max_points,
                          const int32_t* qframe, int Q, const int* stage, const int32_t* loop, const double* Rlq, const double* tlq, const uint8_t* mask,
                          const int32_t* idx, int mcap, const int* nmatch, const double* cam, int32_t* map, int32_t* info) {
  MergeLoop l;
  l.qframe = qframe; l.Q = Q; l.stage = stage; l.loop = loop; l.Rlq = Rlq; l.tlq = tlq; l.mask = mask; l.idx = idx; l.mcap = mcap; l.nmatch = nmatch;
  for (int k = 0; k < 4; ++k) l.cam[k] = cam[k];
  merge_build_host(tables(point_id, xyz, feat, n, size, cap, feat_dim, max_points), l, max_frames, map, info);
}
extern "C" void core_pairs(int32_t* point_id, double* xyz, const float* feat, const int* n, int size, int max_frames, int cap, int feat_dim, int max_points,
                           const int32_t* pairs, int P, int32_t* map, int32_t* info) {
  merge_pairs_host(tables(point_id, xyz, feat, n, size, cap, feat_dim, max_points), pairs, P, map, info);
}
'''


def host_lib(tmpdir):
    """merge_core.h as this tree has it, compiled for the host without contraction"""
    src, so = os.path.join(str(tmpdir), "core.cpp"), os.path.join(str(tmpdir), "libmergecore.so")
    with open(src, "w") as f:
        f.write(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w", "-fPIC", "-shared", "-I" + CSRC, src, "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.core_loop.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4
    lib.core_pairs.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.core_loop.restype = lib.core_pairs.restype = None
    return lib


def feat3(xy):
    """the keypoints as feature rows of 3 columns (score, x, y): what the host statement needs of the 259"""
    f = np.zeros(xy.shape[:2] + (3,), np.float32)
    f[..., 1:] = xy
    return f


def run_host(lib, case):
    """merge_build_host / merge_pairs_host on exactly sized buffers -> (ids, xyz, map, info)"""
    ids, xyz = np.ascontiguousarray(case["ids"], np.int32).copy(), np.ascontiguousarray(case["xyz"], np.float64).copy()
    feat, n = feat3(case["xy"]), np.ascontiguousarray(case["n"], np.int32)
    mp, info = np.full(case["P"], -7, np.int32), np.full(8, -7, np.int32)
    head = (ids.ctypes.data, xyz.ctypes.data, feat.ctypes.data, n.ctypes.data, case["size"], ids.shape[0], ids.shape[1], 3, case["P"])
    if case.get("loop") is not None:
        L = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in case["loop"].items()}
        cam = np.array(L["cam"], np.float64)
        lib.core_loop(*head, L["qframe"].ctypes.data, len(L["qframe"]), L["stage"].ctypes.data, L["loop"].ctypes.data, L["Rlq"].ctypes.data, L["tlq"].ctypes.data,
                      L["mask"].ctypes.data, L["idx"].ctypes.data, L["mcap"], L["nmatch"].ctypes.data, cam.ctypes.data, mp.ctypes.data, info.ctypes.data)
    else:
        pairs = np.ascontiguousarray(case["pairs"], np.int32)
        lib.core_pairs(*head, pairs.ctypes.data, len(pairs), mp.ctypes.data, info.ctypes.data)
    return ids, xyz, mp, info.tolist()


def same(got, want):
    """byte equality of (ids, xyz, map, info)"""
    return (np.asarray(got[0], np.int32).tobytes() == np.asarray(want[0], np.int32).tobytes() and
            np.asarray(got[1], np.float64).tobytes() == np.asarray(want[1], np.float64).tobytes() and
            np.asarray(got[2], np.int32).tobytes() == np.asarray(want[2], np.int32).tobytes() and list(got[3]) == list(want[3]))
