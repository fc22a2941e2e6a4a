// airfe — map-point positions from the stored observations, on the device: Map::TriangulateMappoint (src/map.cc:367-414) over every point of a loaded
// map.  Contract: include/airfe.h ("Map-point triangulation").  The arithmetic is triangulate_core.h's, shared with the host statement; the marking rules
// and the segment starts are covis_core.h's (launch_covis_segments runs in front).  The one atomic below hands out places inside a segment; the segment is
// SORTED before anything reads its order, so no output byte depends on the order in which it landed.  The info and written counters are integer sums
// whose final value is all that is read.
//   tri_fill_kernel     (frame)  the first row of the frame holding each id writes f * cap + i into the id's segment
//   tri_sort_kernel     (one lane per segment ENTRY)  the entry's rank = the entries of its segment below it (they are distinct: one per frame), the
//                       entry goes to sorted[start + rank].  Every lane carries one observation whatever the segment's length (no idle lanes at the
//                       typical 2-20), a segment of n entries costs n reads on each of n lanes — O(n^2 / lanes) at every length, with one code path; the
//                       reads of a segment's lanes are the same addresses (one cache line per 16 entries, broadcast).  The loop runs start[m] ..
//                       start[m + 1]: at most `size` trips, since a frame enters a segment once.
//   tri_point_kernel    (one lane per point)  the core's accumulators over the sorted segment, sequentially, then the solve
//   fill_points_kernel  (frame)  points[f][i] = xyz[id] where the id's status is 0 (and, with only_missing, the stored x is NaN)
#include "common.h"
#include "triangulate_core.h"
#include "kernels.h"
#include "wg_prims.h"

namespace airfe {

namespace {

__global__ __launch_bounds__(256) void tri_fill_kernel(TriangulateArgs a) {
  const int f = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < a.cap; i += 256) {
    const int key = f * a.cap + i;
    const int p = a.packed[key];
    if (!cv_first(p)) continue;
    const int m = cv_id(p);
    const int at = a.start[m] + atomicAdd(a.count + m, 1);
    if (at < a.start[m + 1]) a.seg[at] = key;                      // (always: the segment was sized by the same marks)
  }
}

__global__ __launch_bounds__(256) void tri_sort_kernel(TriangulateArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.start[a.max_points]) return;
  const int key = a.seg[e];
  if ((unsigned)key >= (unsigned)(a.size * a.cap)) return;         // (never: the fill wrote it)
  const int m = cv_id(a.packed[key]);
  if ((unsigned)m >= (unsigned)a.max_points) return;               // (never)
  const int s0 = a.start[m], s1 = a.start[m + 1];
  int rank = 0;
  for (int k = s0; k < s1; ++k) rank += a.seg[k] < key;
  if (s0 + rank < s1) a.sorted[s0 + rank] = key;
}

__global__ __launch_bounds__(256) void tri_point_kernel(TriangulateArgs a) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  int fl[4] = {0, 0, 0, 0};
  if (m < a.max_points) {
    const int s0 = a.size > 0 ? a.start[m] : 0, s1 = a.size > 0 ? a.start[m + 1] : 0;
    TrAcc acc;
    tr_acc_init(&acc);
    for (int k = s0; k < s1; ++k) {
      const int key = a.sorted[k];
      if ((unsigned)key >= (unsigned)(a.size * a.cap)) {             // (never: the sort wrote every place of the segment)
        acc.bad = 1;
        continue;
      }
      const int f = key / a.cap;
      const float* row = a.feat + (size_t)key * a.feat_dim;
      const double* T = a.pose + (size_t)f * 16;
      double P[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) P[q] = T[q];
      tr_acc_add(&acc, a.cami, row[1], row[2], P);
    }
    double x[3];
    const int st = tr_finish(&acc, s1 - s0, a.min_observers, x);
    a.xyz[(size_t)3 * m] = x[0]; a.xyz[(size_t)3 * m + 1] = x[1]; a.xyz[(size_t)3 * m + 2] = x[2];
    a.status[m] = st;
    a.nobs[m] = s1 - s0;
    tr_info_flags(st, fl);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) wave_count_add(fl[k] != 0, a.info + k);
}

__global__ __launch_bounds__(256) void fill_points_kernel(FillPointsArgs a) {
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int n = clamp_count(a.n[f], a.cap);
  const int32_t* ids = a.point_id + (size_t)f * a.cap;
  int w = 0;
  for (int i = t; i < n; i += 256) {
    int ig;
    const int m = cv_row_id(ids, i, n, a.max_points, &ig);
    if (m < 0 || a.status[m] != TR_OK) continue;
    double* p = a.points + ((size_t)f * a.cap + i) * 3;
    if (a.only_missing && !is_nan(p[0])) continue;
    p[0] = a.xyz[(size_t)3 * m]; p[1] = a.xyz[(size_t)3 * m + 1]; p[2] = a.xyz[(size_t)3 * m + 2];
    ++w;
  }
  w = wave_sum(w);                                                 // (a lane writes several rows: a count per lane, not a predicate)
  if (lane == 0 && w) atomicAdd(a.written, w);
}

}  // namespace

void launch_triangulate(const TriangulateArgs& a, hipStream_t st) {
  if (a.size > 0) {
    const long long rows = (long long)a.size * a.cap;
    hipLaunchKernelGGL(tri_fill_kernel, dim3(a.size), dim3(256), 0, st, a);
    hipLaunchKernelGGL(tri_sort_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(tri_point_kernel, dim3((a.max_points + 255) / 256), dim3(256), 0, st, a);
}

int triangulate_point_core(const double* cami, const double* Twc, const float* xy, int n, int min_observers, double* xyz) {
  return triangulate_point_host(cami, Twc, xy, n, min_observers, xyz);
}

void launch_fill_points(const FillPointsArgs& a, hipStream_t st) {
  if (a.size > 0) hipLaunchKernelGGL(fill_points_kernel, dim3(a.size), dim3(256), 0, st, a);
}

}  // namespace airfe
