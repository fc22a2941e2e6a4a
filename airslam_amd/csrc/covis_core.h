// airfe — the covisibility table of a loaded map from the map-point ids of its frames' feature rows: Map::UpdateCovisibilityGraph (src/map.cc:1385-1418)
// on plain arrays.  Contract: include/airfe.h ("Map-point ids and the covisibility build").  One statement for the host and the device: the kernels
// (kernels_covis.hip) call the routines below from their lanes, covis_build_host at the end calls them in loops; tests/covis_ref.py restates the same
// as a Python loop over dicts.  Integers only.
//   valid(f, i)   f < size, i < n[f] and 0 <= point_id[f][i] < max_points
//   obs(m)        the frames with a valid row holding m (a frame is ONE observer however many of its rows hold m)
//   w[f][g]       the number of valid rows i of f with g in obs(point_id[f][i])
//   row f         the pairs (g, w[f][g]) with w > 0, ascending in g
#ifndef AIRFE_COVIS_CORE_H_
#define AIRFE_COVIS_CORE_H_

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "core_common.h"

#define CV_MAX_FRAMES 4096           // frames the build handles: one row's weights are an LDS histogram of this many int32
#define CV_MAX_POINTS (1 << 24)      // map points an id table can be attached for: 8 bytes of work memory per point
#define CV_SCAN_TILE 2048            // points per workgroup of the segment-start scan


// what row i of a frame holds for the build: its id, or -1 (a row past the count is not an id and is never read as one; an id outside
// [0, max_points) is ignored).  *ignored: 1 iff the row is inside the count and its id is neither -1 nor in range.
AIRFE_HD int cv_row_id(const int32_t* frame_ids, int i, int n, int max_points, int* ignored) {
  *ignored = 0;
  if (i >= n) return -1;
  const int id = frame_ids[i];
  if (id >= 0 && id < max_points) return id;
  *ignored = id != -1;
  return -1;
}

// the work table's entry of a row: -1 without a point, otherwise the id and whether the row is the FIRST of its frame that holds it
AIRFE_HD int cv_pack(int id, bool first) { return id < 0 ? -1 : id * 2 + (first ? 1 : 0); }
AIRFE_HD int cv_id(int packed) { return packed < 0 ? -1 : packed >> 1; }
AIRFE_HD bool cv_first(int packed) { return packed >= 0 && (packed & 1); }

// is row i the first of rows 0 .. i that holds ids[i]?  (ids: the frame's cv_row_id values)
AIRFE_HD bool cv_first_occurrence(const int* ids, int i) {
  const int v = ids[i];
  if (v < 0) return false;
  for (int j = 0; j < i; ++j)
    if (ids[j] == v) return false;
  return true;
}

// info i32 [4]: status (0 ok, 1 overflow), entries needed, valid (frame, row) entries, ids ignored as out of range
AIRFE_HD void cv_info(int32_t* info, long long needed, int max_edges, int valid, int ignored) {
  info[0] = needed > max_edges ? 1 : 0;
  info[1] = (int32_t)needed;
  info[2] = valid;
  info[3] = ignored;
}

// The host statement.  point_id [max_frames][cap], n [size]; row_ptr [max_frames + 1], nbr / weight [max_edges], info [4].  Overflow: every row_ptr 0,
// nbr / weight untouched, info[0] = 1.  Frames >= size: empty rows.
inline void covis_build_host(const int32_t* point_id, const int* n, int size, int max_frames, int cap, int max_points, int max_edges, int32_t* row_ptr,
                             int32_t* nbr, int32_t* weight, int32_t* info) {
  std::vector<int> packed((size_t)size * cap, -1), ids(cap);
  std::vector<int> count((size_t)max_points + 1, 0);
  int valid = 0, ignored = 0;
  for (int f = 0; f < size; ++f) {
    const int nf = clamp_count(n[f], cap);
    for (int i = 0; i < cap; ++i) {
      int ig;
      ids[i] = cv_row_id(point_id + (size_t)f * cap, i, nf, max_points, &ig);
      ignored += ig;
      valid += ids[i] >= 0;
    }
    for (int i = 0; i < cap; ++i) {
      const bool first = cv_first_occurrence(ids.data(), i);
      packed[(size_t)f * cap + i] = cv_pack(ids[i], first);
      if (first) ++count[ids[i]];
    }
  }
  std::vector<int> start((size_t)max_points + 1, 0);                // the (point -> frames) segments: start[m] .. start[m + 1]
  for (int m = 0; m < max_points; ++m) start[m + 1] = start[m] + count[m];
  std::vector<int> seg(start[max_points]), cursor(start.begin(), start.end() - 1);
  for (int f = 0; f < size; ++f)
    for (int i = 0; i < cap; ++i)
      if (cv_first(packed[(size_t)f * cap + i])) seg[cursor[cv_id(packed[(size_t)f * cap + i])]++] = f;
  std::vector<int> hist((size_t)(size > 0 ? size : 1));
  long long needed = 0;
  for (int pass = 0; pass < 2; ++pass) {                            // pass 0 counts the entries, pass 1 writes them
    if (pass == 1) {
      cv_info(info, needed, max_edges, valid, ignored);
      if (info[0]) {
        for (int f = 0; f <= max_frames; ++f) row_ptr[f] = 0;
        return;
      }
    }
    int e = 0;
    for (int f = 0; f < size; ++f) {
      std::fill(hist.begin(), hist.end(), 0);
      for (int i = 0; i < cap; ++i) {
        const int m = cv_id(packed[(size_t)f * cap + i]);
        if (m < 0) continue;
        for (int k = start[m]; k < start[m + 1]; ++k) ++hist[seg[k]];
      }
      if (pass == 1) row_ptr[f] = e;
      for (int g = 0; g < size; ++g)
        if (hist[g] > 0) {
          if (pass == 1) { nbr[e] = g; weight[e] = hist[g]; }
          ++e;
        }
    }
    if (pass == 0) needed = e;
    else
      for (int f = size; f <= max_frames; ++f) row_ptr[f] = e;
  }
}

#endif  // AIRFE_COVIS_CORE_H_
