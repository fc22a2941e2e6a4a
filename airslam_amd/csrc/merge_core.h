// airfe — the map-point merge of loop closure on plain arrays: the tail of MapRefiner::RelativatePoseEstimation (src/map_refiner.cc:338-372, :409-459
// without the search of :374-407) and MapRefiner::MergeMappoints / MergeMappointGroup (:603-713).  Contract: include/airfe.h ("Map-point merge").  One
// statement for the host and the device: the kernels (kernels_merge.hip) call the routines below from their lanes, merge_build_host / merge_pairs_host at
// the end call them in loops; tests/merge_ref.py restates the same over dicts and sorted sets.  Doubles, every sum in the order written, no fused
// multiply-adds (the translation units that include this header are compiled with -ffp-contract=off).
//   valid(f, i), size, n[f], max_points   as in covis_core.h (clamp_count).  An id is VALID iff it is in [0, max_points).
//   triangulated(m)   some valid row holding m has a non-NaN x in the point table;  src(m) = the smallest key f * cap + i of such a row
//   Every gate reads the id table and the point table AS THEY WERE BEFORE THE CALL.
//   1 entries     query q with stage[q] == 0, fq = qframe[q], b_f = loop[q], list entry e < min(nmatch[q], mcap), (qi, ci) = idx[q][e]:
//                 dead       fq or b_f outside 0 .. size - 1; qi or ci negative; qi >= n[fq]; ci >= n[b_f]; B = point_id[b_f][ci] not valid
//                 outlier    xyz[b_f][ci].x is not NaN and mask[q][e] == 0 (STATED DIFFERENCE: dropped where the reference searches the inverted file)
//                 epipolar   xyz[b_f][ci].x is NaN and the test of :338-352 fails on p1 = feat[fq][qi].xy, p2 = feat[b_f][ci].xy (STATED DIFFERENCE: the
//                            loop frame's keypoint is row ci, not GetKeypointIdx):
//                              fxi = 1.0 / fx, fyi = 1.0 / fy;  Kit = [fxi 0 0; 0 fyi 0; -(cx * fxi) -(cy * fyi) 1]  (K^-T in closed form)
//                              tx = [0 -t2 t1; t2 0 -t0; -t1 t0 0];  F = ((Kit * tx) * Rlq) * K, every 3 x 3 product element (a0 * b0 + a1 * b1) + a2 * b2
//                              el_r = (F[r][0] * x1 + F[r][1] * y1) + F[r][2];  s = sqrt(el_0 * el_0 + el_1 * el_1);  er = ((x2 * el_0 + y2 * el_1) + el_2) / s
//                              passes iff er < 10.0 (the reference's signed comparison; a NaN er fails)
//                 live       every other entry.  Every feature row counts as having a word (the reference walks word_features).
//   2 adoption    a live entry whose A = point_id[fq][qi] is not valid: row (fq, qi) adopts.  A row adopted by several live entries takes the SMALLEST B, and
//                 all those B are joined.  The adopted row's position is xyz[src(B)] if B is triangulated, else NaN.
//   3 pairs       a live entry with a valid A gives the pair (A, B)
//   4 groups      the connected components over ids of the pairs and of step 2's joins; a group of one is untouched
//   5 best        the smallest triangulated id of the group; without one, its smallest id
//   6 relabel     group G, best b, frame f, R = the valid rows of f whose id AFTER adoption is in G.  Some row of R holds b: those stay, every other row
//                 of R becomes (-1, NaN).  Otherwise, with m* the smallest id in R and i* the first row of f holding m*: row i* becomes (b, xyz[src(b)] or
//                 NaN when b is not triangulated), every other row of R becomes (-1, NaN).  Rows >= n[f], frames >= size and rows of ids in no group are
//                 not touched (an adopted row of an id in no group keeps what step 2 gave it).
//   7 outputs     map[m] = b for a member of a group, else m.  info i32 [8]: live entries, entries dropped as outliers, entries dropped by the epipolar test,
//                 rows adopted (whatever step 6 then makes of them), groups, ids removed (the sum of the group sizes minus the groups), rows relabelled to
//                 a best, rows cleared.  The pair form: pairs taken, pairs ignored (an id not valid), 0, 0, then the same.
// The position read for a relabelled or adopted row, xyz[src(b)], is a row that holds the best of its group or an id in no group: no call changes it.
#ifndef AIRFE_MERGE_CORE_H_
#define AIRFE_MERGE_CORE_H_

#include <math.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "covis_core.h"

#define MG_MAX_FRAMES CV_MAX_FRAMES  // frames a merge handles: the key f * cap + i is an int32 at 4096 frames x 1024 rows
#define MG_MAX_QUERIES 4096
#define MG_MAX_MATCHES 1024          // mcap
#define MG_NONE 0x7fffffff           // src of an id without a triangulated row; the best of a group without a triangulated member

enum { MG_DEAD = 0, MG_OUTLIER = 1, MG_EPIPOLAR = 2, MG_PAIR = 3, MG_ADOPT = 4 };
enum { MG_KEEP = 0, MG_BEST = 1, MG_CLEAR = 2 };
enum { MG_I_LIVE = 0, MG_I_OUTLIER, MG_I_EPIPOLAR, MG_I_ADOPTED, MG_I_GROUPS, MG_I_REMOVED, MG_I_RELABELLED, MG_I_CLEARED, MG_INFO };

// the database's tables as the merge reads and writes them
struct MergeTables {
  int32_t* point_id = nullptr; double* xyz = nullptr;                        // [max_frames][cap], [max_frames][cap][3]: changed in place by step 6
  const float* feat = nullptr; const int* n = nullptr;                       // [max_frames][cap][feat_dim] (x, y at columns 1, 2), [max_frames]
  int size = 0, cap = 0, feat_dim = 0, max_points = 0;
};
// airfe_loop_detect_batch_dev's outputs as step 1 reads them
struct MergeLoop {
  const int32_t* qframe = nullptr; int Q = 0;
  const int* stage = nullptr; const int32_t* loop = nullptr; const double *Rlq = nullptr, *tlq = nullptr;      // [Q], [Q], [Q][9], [Q][3]
  const uint8_t* mask = nullptr; const int32_t* idx = nullptr; int mcap = 0; const int* nmatch = nullptr;      // [Q][mcap], [Q][mcap][2], [Q]
  double cam[4] = {0, 0, 0, 0};                                              // fx, fy, cx, cy
};

AIRFE_HD bool mg_valid_id(int id, int max_points) { return id >= 0 && id < max_points; }
AIRFE_HD bool mg_cam_ok(const double* cam) { return is_finite(cam[0]) && is_finite(cam[1]) && cam[0] != 0.0 && cam[1] != 0.0; }

AIRFE_HD void mg_mul3(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// F = ((K^-T * [tlq]x) * Rlq) * K, row-major
AIRFE_HD void mg_fundamental(const double* cam, const double* Rlq, const double* tlq, double* F) {
  const double fxi = 1.0 / cam[0], fyi = 1.0 / cam[1];
  const double Kit[9] = {fxi, 0.0, 0.0, 0.0, fyi, 0.0, -(cam[2] * fxi), -(cam[3] * fyi), 1.0};
  const double tx[9] = {0.0, -tlq[2], tlq[1], tlq[2], 0.0, -tlq[0], -tlq[1], tlq[0], 0.0};
  const double K[9] = {cam[0], 0.0, cam[2], 0.0, cam[1], cam[3], 0.0, 0.0, 1.0};
  double T1[9], T2[9];
  mg_mul3(Kit, tx, T1);
  mg_mul3(T1, Rlq, T2);
  mg_mul3(T2, K, F);
}

// check_epipolar (:342-352): p1 on the query frame, p2 on the loop frame
AIRFE_HD bool mg_epipolar(const double* F, double x1, double y1, double x2, double y2) {
  const double el0 = (F[0] * x1 + F[1] * y1) + F[2], el1 = (F[3] * x1 + F[4] * y1) + F[5], el2 = (F[6] * x1 + F[7] * y1) + F[8];
  const double s = sqrt(el0 * el0 + el1 * el1);
  const double er = ((x2 * el0 + y2 * el1) + el2) / s;
  return er < 10.0;
}

// step 1 for entry (q, e), e < clamp_count(nmatch[q], mcap) of a query with stage 0 -> MG_DEAD .. MG_ADOPT; for MG_PAIR *A and *B, for MG_ADOPT *B and
// *row = the adopting row's key
AIRFE_HD int mg_entry(const MergeTables& t, const MergeLoop& l, int q, int e, int* A, int* B, int* row) {
  const int fq = l.qframe[q], bf = l.loop[q];
  if (fq < 0 || fq >= t.size || bf < 0 || bf >= t.size) return MG_DEAD;
  const size_t at = (size_t)q * l.mcap + e;
  const int qi = l.idx[2 * at], ci = l.idx[2 * at + 1];
  if (qi < 0 || ci < 0 || qi >= clamp_count(t.n[fq], t.cap) || ci >= clamp_count(t.n[bf], t.cap)) return MG_DEAD;
  const size_t rq = (size_t)fq * t.cap + qi, rl = (size_t)bf * t.cap + ci;
  const int b = t.point_id[rl];
  if (!mg_valid_id(b, t.max_points)) return MG_DEAD;
  if (!is_nan(t.xyz[3 * rl])) {
    if (l.mask[at] == 0) return MG_OUTLIER;
  } else {
    double F[9];
    mg_fundamental(l.cam, l.Rlq + 9 * (size_t)q, l.tlq + 3 * (size_t)q, F);
    const float* p1 = t.feat + rq * t.feat_dim;
    const float* p2 = t.feat + rl * t.feat_dim;
    if (!mg_epipolar(F, (double)p1[1], (double)p1[2], (double)p2[1], (double)p2[2])) return MG_EPIPOLAR;
  }
  const int a = t.point_id[rq];
  *B = b;
  if (mg_valid_id(a, t.max_points)) {
    *A = a;
    return MG_PAIR;
  }
  *row = (int)rq;
  return MG_ADOPT;
}

// what row i of a frame holds after adoption: its own valid id; else the id staged for it (-1: none); -1 past the count
AIRFE_HD int mg_row_id(int own, int staged, int i, int n, int max_points) {
  if (i >= n) return -1;
  if (mg_valid_id(own, max_points)) return own;
  return mg_valid_id(staged, max_points) ? staged : -1;
}

// step 6 for row i of a frame: ids = the rows' mg_row_id, grp = the group of each (its smallest id; -1: in no group), b = the best of grp[i]
AIRFE_HD int mg_row_decision(const int* ids, const int* grp, int rows, int i, int b) {
  const int g = grp[i];
  if (g < 0) return MG_KEEP;
  bool hasb = false;
  int mstar = MG_NONE, istar = -1;
  for (int j = 0; j < rows; ++j) {
    if (grp[j] != g) continue;
    hasb = hasb || ids[j] == b;
    if (ids[j] < mstar) { mstar = ids[j]; istar = j; }
  }
  if (hasb) return ids[i] == b ? MG_KEEP : MG_CLEAR;
  return i == istar ? MG_BEST : MG_CLEAR;
}

// Steps 4 - 7, sequential.  pairs: valid ids; staged [max_frames][cap] or empty: the id each adopting row takes (-1: none), its joins already among the
// pairs.  map [max_points], info [8]: entries 3 .. 7 are written here.
inline void merge_apply_host(const MergeTables& t, const std::vector<std::pair<int, int>>& pairs, const std::vector<int>& staged, int32_t* map,
                             int32_t* info) {
  const int P = t.max_points;
  std::vector<int> parent(P), src(P, MG_NONE), bestv(P, MG_NONE), members(P, 0);
  std::vector<char> touched(P, 0);
  for (int m = 0; m < P; ++m) parent[m] = m;
  auto find = [&](int u) {
    int r = u;
    while (parent[r] != r) r = parent[r];
    while (parent[u] != r) { const int nx = parent[u]; parent[u] = r; u = nx; }
    return r;
  };
  for (const auto& p : pairs) {
    const int u = find(p.first), v = find(p.second);
    if (u != v) parent[u > v ? u : v] = u > v ? v : u;             // the root of a group is its smallest id
    touched[p.first] = touched[p.second] = 1;
  }
  int adopted = 0;
  if (!staged.empty())
    for (int f = 0; f < t.size; ++f)
      for (int i = 0, nf = clamp_count(t.n[f], t.cap); i < nf; ++i) {
        const size_t r = (size_t)f * t.cap + i;
        if (!mg_valid_id(t.point_id[r], P) && mg_valid_id(staged[r], P)) { touched[staged[r]] = 1; ++adopted; }
      }
  for (int f = 0; f < t.size; ++f)
    for (int i = 0, nf = clamp_count(t.n[f], t.cap); i < nf; ++i) {
      const size_t r = (size_t)f * t.cap + i;
      const int m = t.point_id[r];
      if (mg_valid_id(m, P) && touched[m] && !is_nan(t.xyz[3 * r]) && src[m] == MG_NONE) src[m] = (int)r;      // ascending keys: the first is the smallest
    }
  int groups = 0, removed = 0;
  for (int m = 0; m < P; ++m) {
    if (!touched[m]) continue;
    const int r = find(m);
    ++members[r];
    if (src[m] != MG_NONE && bestv[r] == MG_NONE) bestv[r] = m;    // ascending ids: the first is the smallest
  }
  for (int m = 0; m < P; ++m) {
    map[m] = m;
    if (!touched[m]) continue;
    const int r = find(m);
    if (members[r] >= 2) map[m] = bestv[r] != MG_NONE ? bestv[r] : r;
    if (r == m && members[r] >= 2) { ++groups; removed += members[r] - 1; }
  }
  int relabelled = 0, cleared = 0;
  std::vector<int> ids(t.cap), grp(t.cap), what(t.cap);
  for (int f = 0; f < t.size; ++f) {
    const int nf = clamp_count(t.n[f], t.cap);
    bool any = false;
    for (int i = 0; i < nf; ++i) {
      const size_t r = (size_t)f * t.cap + i;
      ids[i] = mg_row_id(t.point_id[r], staged.empty() ? -1 : staged[r], i, nf, P);
      grp[i] = -1;
      if (ids[i] >= 0 && touched[ids[i]] && members[find(ids[i])] >= 2) grp[i] = find(ids[i]);
      any = any || grp[i] >= 0 || (ids[i] >= 0 && ids[i] != t.point_id[r]);
    }
    if (!any) continue;
    for (int i = 0; i < nf; ++i) what[i] = mg_row_decision(ids.data(), grp.data(), nf, i, grp[i] >= 0 ? map[ids[i]] : -1);
    for (int i = 0; i < nf; ++i) {
      const size_t r = (size_t)f * t.cap + i;
      const bool adopting = ids[i] >= 0 && ids[i] != t.point_id[r];      // (the row held no valid id and takes the staged one)
      if (what[i] == MG_KEEP && !adopting) continue;
      const int id = what[i] == MG_CLEAR ? -1 : (what[i] == MG_BEST ? map[ids[i]] : ids[i]);
      const int from = id >= 0 ? src[id] : MG_NONE;
      t.point_id[r] = id;
      for (int k = 0; k < 3; ++k) t.xyz[3 * r + k] = from != MG_NONE ? t.xyz[3 * (size_t)from + k] : quiet_nan();
      relabelled += what[i] == MG_BEST;
      cleared += what[i] == MG_CLEAR;
    }
  }
  info[MG_I_ADOPTED] = adopted; info[MG_I_GROUPS] = groups; info[MG_I_REMOVED] = removed; info[MG_I_RELABELLED] = relabelled; info[MG_I_CLEARED] = cleared;
}

// The host statement of airfe_bowdb_merge_points_dev: steps 4 - 7 on the pair list [P][2]
inline void merge_pairs_host(const MergeTables& t, const int32_t* pairs, int P, int32_t* map, int32_t* info) {
  std::vector<std::pair<int, int>> ok;
  int ignored = 0;
  for (int k = 0; k < P; ++k) {
    if (mg_valid_id(pairs[2 * k], t.max_points) && mg_valid_id(pairs[2 * k + 1], t.max_points)) ok.emplace_back(pairs[2 * k], pairs[2 * k + 1]);
    else ++ignored;
  }
  info[MG_I_LIVE] = (int32_t)ok.size(); info[MG_I_OUTLIER] = ignored; info[MG_I_EPIPOLAR] = 0;
  merge_apply_host(t, ok, std::vector<int>(), map, info);
}

// The host statement of airfe_bowdb_loop_merge_batch_dev: steps 1 - 7.  max_frames: the tables' frames (the staging's size).
inline void merge_build_host(const MergeTables& t, const MergeLoop& l, int max_frames, int32_t* map, int32_t* info) {
  std::vector<std::pair<int, int>> pairs;
  std::vector<int> staged((size_t)max_frames * t.cap, -1);
  std::vector<std::pair<int, int>> adopts;                         // (row, B)
  int count[5] = {0, 0, 0, 0, 0};
  for (int q = 0; q < l.Q; ++q) {
    if (l.stage[q] != 0) continue;
    for (int e = 0, ne = clamp_count(l.nmatch[q], l.mcap); e < ne; ++e) {
      int A = -1, B = -1, row = -1;
      const int kind = mg_entry(t, l, q, e, &A, &B, &row);
      ++count[kind];
      if (kind == MG_PAIR) pairs.emplace_back(A, B);
      if (kind == MG_ADOPT) {
        adopts.emplace_back(row, B);
        if (staged[row] < 0 || B < staged[row]) staged[row] = B;
      }
    }
  }
  for (const auto& a : adopts) pairs.emplace_back(a.second, staged[a.first]);
  info[MG_I_LIVE] = count[MG_PAIR] + count[MG_ADOPT]; info[MG_I_OUTLIER] = count[MG_OUTLIER]; info[MG_I_EPIPOLAR] = count[MG_EPIPOLAR];
  merge_apply_host(t, pairs, staged, map, info);
}

#endif  // AIRFE_MERGE_CORE_H_
