// airfe — loop detection over a loaded map (MapRefiner::LoopDetection, src/map_refiner.cc:65-235, and RelativatePoseEstimation, :237-333) on plain arrays:
// what is NEW next to the relocalisation path.  Contract: include/airfe.h ("Stored queries against their predecessors", "Loop detection composite").
// One statement for the host and the device: the kernels (kernels_loopdet.hip) call the routines below from their lanes, the host routines at the end
// call them in loops; tests/loopdet_ref.py restates the same in Python floats.  fp64, sums sequential in the order written; compile without FMA
// contraction.
//   odometry prefix    odom[f] = the path length up to frame f (:66-81)
//   prefix selection   frame fq against frames 0 .. fq - 1 only: the database as it was when the reference queried it (AddFrame comes after, :88-89)
//   constraint rule    a list entry (qi, ci) of the winner b becomes a constraint iff xyz[b][ci] exists; u = u_right[fq][qi] if > 0, else -1 (:266-300)
//   stages             0 ok, 1 no candidate, 2 no group, 3 no winner / too few matches, 4 too few constraints, 5 too few inliers
//   relative pose      Rlq = Rwl^T Rwq, tlq = Rwl^T (twq - twl) (:327-333)
#ifndef AIRFE_LOOPDET_CORE_H_
#define AIRFE_LOOPDET_CORE_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "core_common.h"

#define LD_MAX_QUERIES 4096     // stored queries per call
#define LD_MAX_FRAMES 4096      // frames the composite handles (the grouping's candidate capacity, the odometry kernel's LDS)

// |b - a| as :76 computes it
AIRFE_HD double ld_step(const double* a, const double* b) {
  const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// odom[0] = +0, odom[f] = odom[f - 1] + step[f]: sequential, ascending f (step[f] = |pos[f] - pos[f - 1]|, step[0] unused)
AIRFE_HD void ld_prefix(const double* step, int n, double* odom) {
  double s = 0.0;
  for (int f = 0; f < n; ++f) {
    if (f > 0) s += step[f];
    odom[f] = s;
  }
}

// std::max(static_cast<int>(max_sharing_words * 0.5f), 8) (:108): a float product, truncated
AIRFE_HD int ld_threshold(int max_sharing, float ratio, int min_words) {
  const float prod = (float)max_sharing * ratio;
  const int t = (int)prod;
  return t > min_words ? t : min_words;
}

// does frame f exist for the query fq?  fq outside 0 .. size - 1: nothing does
AIRFE_HD bool ld_exists(int f, int fq, int size) { return fq >= 0 && fq < size && f >= 0 && f < fq; }

// is f a neighbour in row fq of the covisibility CSR, at ANY weight (covi_frames.count(fsw), :115)?  Rows ascend strictly in nbr.
AIRFE_HD bool ld_covisible(const int32_t* row_ptr, const int32_t* nbr, int rows, int fq, int f) {
  if (fq < 0 || fq >= rows) return false;
  int lo = row_ptr[fq], hi = row_ptr[fq + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nbr[mid] < f) lo = mid + 1; else hi = mid;
  }
  return lo < row_ptr[fq + 1] && nbr[lo] == f;
}

// the candidate predicate for a frame that exists (f < fq), :113-120; (a frame without a common word is absent from frame_sharing_words)
AIRFE_HD bool ld_candidate(int sharing, int thr, bool covisible) { return sharing > 0 && sharing >= thr && !covisible; }

// the constraint of list entry (qi, ci): point = xyz[b][ci], feat_row = the query's row qi ([259]: score, x, y, ...), u_right = u_right[fq][qi].
// Returns whether there is one; obs = (x, y, u), u > 0 iff stereo (the convention of "Frame optimisation")
AIRFE_HD bool ld_constraint(const double* point, const float* feat_row, double u_right, double* X, double* obs) {
  if (isnan(point[0])) return false;
  X[0] = point[0]; X[1] = point[1]; X[2] = point[2];
  obs[0] = (double)feat_row[1];
  obs[1] = (double)feat_row[2];
  obs[2] = u_right > 0.0 ? u_right : -1.0;
  return true;
}

// the gates before the constraints: :101 / :122, :174, :232 (STRICTLY more than min_matches)
AIRFE_HD int ld_stage_before(int ncand, int gstatus, int ngroups, int best, int size, int nmatch, int min_matches) {
  if (ncand <= 0) return 1;
  if (gstatus != 0 || ngroups <= 0) return 2;
  if (best < 0 || best >= size || nmatch <= min_matches) return 3;
  return 0;
}
// ... and behind them: :301, :308
AIRFE_HD int ld_stage(int before, int ncons, int min_points, int num, int min_inliers) {
  if (before) return before;
  if (ncons < min_points) return 4;
  return num < min_inliers ? 5 : 0;
}

// Twl, Twq [16] row-major -> Rlq [9] row-major, tlq [3]
AIRFE_HD void ld_relative_pose(const double* Twl, const double* Twq, double* Rlq, double* tlq) {
  const double d0 = Twq[3] - Twl[3], d1 = Twq[7] - Twl[7], d2 = Twq[11] - Twl[11];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rlq[3 * i + j] = (Twl[i] * Twq[j] + Twl[4 + i] * Twq[4 + j]) + Twl[8 + i] * Twq[8 + j];
    tlq[i] = (Twl[i] * d0 + Twl[4 + i] * d1) + Twl[8 + i] * d2;
  }
}
AIRFE_HD void ld_no_relative_pose(double* Rlq, double* tlq) {
  for (int k = 0; k < 9; ++k) Rlq[k] = (k % 4 == 0) ? 1.0 : 0.0;
  tlq[0] = tlq[1] = tlq[2] = 0.0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// pos [n][3] -> odom [n]
inline void loopdet_odometry_host(const double* pos, int n, double* odom) {
  std::vector<double> step(n > 0 ? n : 0, 0.0);
  for (int f = 1; f < n; ++f) step[f] = ld_step(pos + 3 * (size_t)(f - 1), pos + 3 * (size_t)f);
  ld_prefix(step.data(), n, odom);
}

// sharing and L1 score of two vectors (ids ascending): v1 = the stored frame's, v2 = the query's, the common words in ascending word id
inline void loopdet_share_score_host(const uint32_t* i1, const double* x1, int n1, const uint32_t* i2, const double* x2, int n2, int* sharing, double* score) {
  int a = 0, b = 0, sh = 0;
  double s = 0.0;
  while (a < n1 && b < n2) {
    if (i1[a] == i2[b]) {
      s += (fabs(x1[a] - x2[b]) - fabs(x1[a])) - fabs(x2[b]);
      ++sh; ++a; ++b;
    } else if (i1[a] < i2[b]) ++a;
    else ++b;
  }
  *sharing = sh;
  *score = -s / 2.0;
}

// One stored query on the host over a database of `size` frames (ids / vals [size][cap], nw [size]).  row_ptr == nullptr: nothing is covisible.
// cand_* [ccap]: the first min(*ncand, ccap) candidates in ascending frame; dense [size] or nullptr: sharing below fq, 0 from fq on.
inline void loopdet_select_host(const uint32_t* ids, const double* vals, const int* nw, int size, int cap, int fq, float ratio, int min_words,
                                const int32_t* row_ptr, const int32_t* nbr, int rows, int32_t* cand_frame, int32_t* cand_sharing, double* cand_score, int ccap,
                                int* ncand, int* max_sharing, int32_t* dense) {
  *ncand = 0;
  *max_sharing = 0;
  if (dense) for (int f = 0; f < size; ++f) dense[f] = 0;
  if (fq < 0 || fq >= size) return;
  int ms = 0;
  for (int f = 0; f < fq; ++f) {
    int sh;
    double sc;
    loopdet_share_score_host(ids + (size_t)f * cap, vals + (size_t)f * cap, nw[f], ids + (size_t)fq * cap, vals + (size_t)fq * cap, nw[fq], &sh, &sc);
    if (dense) dense[f] = sh;
    if (sh > ms) ms = sh;
  }
  *max_sharing = ms;
  const int thr = ld_threshold(ms, ratio, min_words);
  int n = 0;
  for (int f = 0; f < fq; ++f) {
    int sh;
    double sc;
    loopdet_share_score_host(ids + (size_t)f * cap, vals + (size_t)f * cap, nw[f], ids + (size_t)fq * cap, vals + (size_t)fq * cap, nw[fq], &sh, &sc);
    if (!ld_exists(f, fq, size) || !ld_candidate(sh, thr, row_ptr && ld_covisible(row_ptr, nbr, rows, fq, f))) continue;
    if (n < ccap) { cand_frame[n] = f; cand_sharing[n] = sh; cand_score[n] = sc; }
    ++n;
  }
  *ncand = n;
}

// the winner's list (qi, ci) [m] -> constraints in list order: X / obs [<= m][3], map [<= m] = the list entry of constraint i.  xyz_b [cap][3] = the
// winner's points, feat_q [cap][259] / u_right_q [cap] = the query's rows.  Returns the count.
inline int loopdet_constraints_host(const int32_t* idx, int m, const double* xyz_b, const float* feat_q, const double* u_right_q, int cap, double* X,
                                    double* obs, int* map) {
  int n = 0;
  for (int j = 0; j < m; ++j) {
    const int qi = idx[2 * j], ci = idx[2 * j + 1];
    if (qi < 0 || qi >= cap || ci < 0 || ci >= cap) continue;
    if (!ld_constraint(xyz_b + 3 * (size_t)ci, feat_q + 259 * (size_t)qi, u_right_q[qi], X + 3 * (size_t)n, obs + 3 * (size_t)n)) continue;
    map[n++] = j;
  }
  return n;
}
#endif

#endif  // AIRFE_LOOPDET_CORE_H_
