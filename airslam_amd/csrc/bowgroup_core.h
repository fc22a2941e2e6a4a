// airfe — the GROUPING between the BoW scores and the candidates of MapUser::Relocalization (src/map_user.cc:177-270, 331, 347-363) and
// MapRefiner::LoopDetection (src/map_refiner.cc:132-214) on plain arrays.  Contract: include/airfe.h ("Grouping").  One statement for the host and the
// device: the kernel (kernels_bowgroup.hip) calls the per-candidate, per-group and ranking routines below from its lanes, bowgroup_host calls them in a
// loop; tests/bowgroup_ref.py restates the same with dicts.  fp64, sums sequential in the order written; compile without FMA contraction.
//   candidate list   frame [n] ascending, score [n]: airfe_bowdb_query_batch_dev's output = the reference's frame_scores map
//   covisibility     CSR: row_ptr [rows + 1], nbr / weight [row_ptr[rows]], every row strictly ascending in nbr, the frame's own entry included as it is
//   a "slot" is an index into the candidate list; ascending slot = ascending frame index = the order every std::map / std::set iteration takes here
#ifndef AIRFE_BOWGROUP_CORE_H_
#define AIRFE_BOWGROUP_CORE_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "core_common.h"

#define BG_MAX_CAND 4096        // candidates per query the kernel holds in LDS
#define BG_MODE_RELOC 0
#define BG_MODE_LOOP 1
#define BG_OK 0
#define BG_NO_GROUP 1           // best_group_score < 0 (map_user.cc:219, map_refiner.cc:174); a query without candidates ends here too
#define BG_OVERFLOW 2           // ncand > ccap: the list is incomplete, nothing is grouped
#define BG_MIN_WEIGHT 10        // kv.second > 10
#define BG_TOP 5                // CoviFrameScoreNum

// slot of frame f in the ascending list, or -1
AIRFE_HD int bg_find(const int32_t* frame, int n, int f) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (frame[mid] < f) lo = mid + 1; else hi = mid;
  }
  return lo < n && frame[lo] == f ? lo : -1;
}

// the covisibility row of frame f: entries [*e0, *e1)
AIRFE_HD void bg_row(const int32_t* row_ptr, int rows, int f, int* e0, int* e1) {
  if (f < 0 || f >= rows) { *e0 = *e1 = 0; return; }
  *e0 = row_ptr[f];
  *e1 = row_ptr[f + 1];
}

// map_user.cc:183-206 for candidate slot i: the group's score and its deputy's slot
AIRFE_HD void bg_candidate(const int32_t* frame, const double* score, int n, const int32_t* row_ptr, const int32_t* nbr, const int32_t* weight, int rows, int i,
                        double* gscore, int* deputy) {
  double s = 0.0 + score[i], ds = score[i];       // group_score starts at 0 (map_user.h:24): a score of -0 enters as +0
  int d = i, e0, e1;
  bg_row(row_ptr, rows, frame[i], &e0, &e1);
  for (int e = e0; e < e1; ++e) {
    if (weight[e] <= BG_MIN_WEIGHT) continue;
    const int j = bg_find(frame, n, nbr[e]);
    if (j < 0) continue;
    const double sj = score[j];
    s += sj;                                      // the frame's own entry is an entry like any other: its score is added again
    if (sj > ds) { d = j; ds = sj; }
  }
  *gscore = s;
  *deputy = d;
}

// map_user.cc:208-216 over the whole list, in list order: group_of[d] = the slot of the candidate whose group is stored under deputy slot d (-1: none).
// Returns best_group_score.  Sequential by contract: a later candidate replaces a stored group only with a strictly larger score.
AIRFE_HD double bg_replace(const double* gscore, const int* deputy, int n, int* group_of) {
  double best = -1.0;
  for (int i = 0; i < n; ++i) {
    const int d = deputy[i];
    const double s = gscore[i];
    const int g = group_of[d];
    if (g < 0 || gscore[g] < s) {
      group_of[d] = i;
      if (s > best) best = s;
    }
  }
  return best;
}

// is (s, p) ranked behind (ps, pp)?  Ranking: score descending, ties to the lower position.
AIRFE_HD bool bg_behind(double s, int p, double ps, int pp) { return s < ps || (s == ps && p > pp); }
// is (s, p) ranked before (bs, bp)?  bp < 0: there is no (bs, bp) yet
AIRFE_HD bool bg_before(double s, int p, double bs, int bp) { return bp < 0 || s > bs || (s == bs && p < bp); }

// map_user.cc:224-240 for the group candidate slot i stored: its members are the candidate and its qualifying neighbours (a std::set: the own entry
// counts once); more than 5 members: the five largest scores in descending order, otherwise every score in ascending frame index; from +0.
AIRFE_HD double bg_resum(const int32_t* frame, const double* score, int n, const int32_t* row_ptr, const int32_t* nbr, const int32_t* weight, int rows, int i) {
  const int f = frame[i];
  const double si = score[i];
  int e0, e1, members = 1;
  bg_row(row_ptr, rows, f, &e0, &e1);
  for (int e = e0; e < e1; ++e)
    if (weight[e] > BG_MIN_WEIGHT && nbr[e] != f && bg_find(frame, n, nbr[e]) >= 0) ++members;
  double sum = 0.0;
  if (members <= BG_TOP) {
    bool placed = false;
    for (int e = e0; e < e1; ++e) {
      if (weight[e] <= BG_MIN_WEIGHT) continue;
      const int j = bg_find(frame, n, nbr[e]);
      if (j < 0) continue;
      if (!placed && nbr[e] >= f) {
        if (nbr[e] > f) sum += si;
        placed = true;
      }
      sum += score[j];
    }
    if (!placed) sum += si;
    return sum;
  }
  double ps = 0.0;
  int pp = -1;
  for (int r = 0; r < BG_TOP; ++r) {              // selection by (score descending, frame ascending): equal scores add the same value
    double bs = si;
    int bp = (r == 0 || bg_behind(si, f, ps, pp)) ? f : -1;
    for (int e = e0; e < e1; ++e) {
      if (weight[e] <= BG_MIN_WEIGHT || nbr[e] == f) continue;
      const int j = bg_find(frame, n, nbr[e]);
      if (j < 0) continue;
      const double sj = score[j];
      if ((r == 0 || bg_behind(sj, nbr[e], ps, pp)) && bg_before(sj, nbr[e], bs, bp)) { bs = sj; bp = nbr[e]; }
    }
    if (bp < 0) break;
    sum += bs;
    ps = bs;
    pp = bp;
  }
  return sum;
}

// map_refiner.cc:177-191: is the deputy farther from the query than max_dist?
AIRFE_HD bool bg_far(const double* qpos, const double* p, double max_dist) {
  const double dx = qpos[0] - p[0], dy = qpos[1] - p[1], dz = qpos[2] - p[2];
  return sqrt((dx * dx + dy * dy) + dz * dz) > max_dist;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One query on the host.  extra [n_extra] or nullptr (relocalisation: added to a group's score by its deputy's frame index); pos [pos_rows][3], qpos [3],
// max_dist (loop form).  out_frame / out_score [K] (-1 / 0.0 padded), *ngroups = the groups left after the filters (may exceed K), *status = BG_*.
inline void bowgroup_host(int mode, const int32_t* frame, const double* score, int ncand, int ccap, const int32_t* row_ptr, const int32_t* nbr,
                          const int32_t* weight, int rows, const double* extra, int n_extra, const double* pos, int pos_rows, const double* qpos,
                          double max_dist, int K, int32_t* out_frame, double* out_score, int* ngroups, int* status) {
  for (int k = 0; k < K; ++k) { out_frame[k] = -1; out_score[k] = 0.0; }
  *ngroups = 0;
  if (ncand > ccap) { *status = BG_OVERFLOW; return; }
  const int n = ncand < 0 ? 0 : ncand;
  std::vector<double> gscore(n), fin(n);
  std::vector<int> deputy(n), group_of(n, -1);
  for (int i = 0; i < n; ++i) bg_candidate(frame, score, n, row_ptr, nbr, weight, rows, i, &gscore[i], &deputy[i]);
  const double best_group = bg_replace(gscore.data(), deputy.data(), n, group_of.data());
  if (best_group < 0) { *status = BG_NO_GROUP; return; }
  *status = BG_OK;
  int stored = 0;
  double best = 0.0;
  for (int d = 0; d < n; ++d) {
    if (group_of[d] < 0) continue;
    if (mode == BG_MODE_RELOC) {
      fin[d] = bg_resum(frame, score, n, row_ptr, nbr, weight, rows, group_of[d]);
      if (best < fin[d]) best = fin[d];
    } else {
      fin[d] = gscore[group_of[d]];
      if (frame[d] >= 0 && frame[d] < pos_rows && bg_far(qpos, pos + 3 * (size_t)frame[d], max_dist)) { group_of[d] = -1; continue; }
    }
    ++stored;
  }
  if (mode == BG_MODE_LOOP) best = best_group;    // taken before the distance filter, as in the reference
  const double thr = best * 0.5;
  int left = 0;
  for (int d = 0; d < n; ++d) {
    if (group_of[d] < 0) continue;
    if (stored > 3 && fin[d] < thr) { group_of[d] = -1; continue; }
    if (mode == BG_MODE_RELOC && extra && frame[d] >= 0 && frame[d] < n_extra) fin[d] += extra[frame[d]];
    ++left;
  }
  *ngroups = left;
  double ps = 0.0;
  int pp = -1;
  for (int r = 0; r < K; ++r) {
    double bs = 0.0;
    int bp = -1;
    for (int d = 0; d < n; ++d)
      if (group_of[d] >= 0 && (r == 0 || bg_behind(fin[d], d, ps, pp)) && bg_before(fin[d], d, bs, bp)) { bs = fin[d]; bp = d; }
    if (bp < 0) break;
    out_frame[r] = frame[bp];
    out_score[r] = bs;
    ps = bs;
    pp = bp;
  }
}
#endif

#endif  // AIRFE_BOWGROUP_CORE_H_
