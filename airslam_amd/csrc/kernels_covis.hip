// airfe — the covisibility table built on the device from the stored map-point ids: Map::UpdateCovisibilityGraph (src/map.cc:1385-1418) for a loaded
// map.  Contract: include/airfe.h ("Map-point ids and the covisibility build").  The rules are covis_core.h's, shared with the host statement.  Integers
// only.  The atomics below add 1 to counters whose final VALUE is all that is read (counts, histogram cells) or hand out places inside a segment whose
// ORDER nothing reads (only how often a frame occurs in it): no output byte depends on the order in which they land.
//   covis_mark_kernel       (frame)  the rows' ids into LDS; the first row of the frame holding each id is marked and adds 1 to count[id]; the work
//                           table gets (id, first) per row; the valid and ignored totals
//   covis_tile_sum_kernel   (tile of 2048 points)  the tile's sum of counts
//   covis_tile_scan_kernel  (one workgroup)  the tile sums -> tile offsets
//   covis_start_kernel      (tile)  start[m] = the exclusive prefix of count, start[max_points] = the total; count[m] = 0 again (the fill's cursor)
//   covis_fill_kernel       (frame)  frame f into the segment of every id it holds (once per id)
//   covis_count_kernel      (frame)  w[f][.] into an LDS histogram over the frames: the segment of every valid row, duplicates included; the non-zeros
//   covis_rows_kernel       (one workgroup)  the row counts -> row_ptr; overflow -> every row_ptr 0; info
//   covis_emit_kernel       (frame)  the histogram again, compacted in ascending g by ballot + prefix
#include "common.h"
#include "covis_core.h"
#include "kernels.h"
#include "wg_prims.h"

namespace airfe {

namespace {

__global__ __launch_bounds__(256) void covis_mark_kernel(CovisArgs a) {
  __shared__ int ids[BOW_MAX_FEATURES];
  __shared__ int tot[2];
  const int f = blockIdx.x, t = threadIdx.x;
  const int n = clamp_count(a.n[f], a.cap);
  const int32_t* row = a.point_id + (size_t)f * a.cap;
  if (t < 2) tot[t] = 0;
  int valid = 0, ignored = 0;
  for (int i = t; i < a.cap; i += 256) {
    int ig;
    const int id = cv_row_id(row, i, n, a.max_points, &ig);
    ids[i] = id;
    ignored += ig;
    valid += id >= 0;
  }
  __syncthreads();
  for (int i = t; i < a.cap; i += 256) {
    const bool first = cv_first_occurrence(ids, i);
    a.packed[(size_t)f * a.cap + i] = cv_pack(ids[i], first);
    if (first) atomicAdd(a.count + ids[i], 1);
  }
  if (valid) atomicAdd(&tot[0], valid);
  if (ignored) atomicAdd(&tot[1], ignored);
  __syncthreads();
  if (t < 2 && tot[t]) atomicAdd(a.acc + t, tot[t]);
}

__global__ __launch_bounds__(256) void covis_tile_sum_kernel(CovisArgs a) {
  __shared__ int wsum[4];
  const int t = threadIdx.x, P = a.max_points + 1;
  const size_t base = (size_t)blockIdx.x * CV_SCAN_TILE;
  int s = 0;
  for (int k = 0; k < CV_SCAN_TILE / 256; ++k) {
    const size_t m = base + (size_t)k * 256 + t;
    if (m < (size_t)P) s += a.count[m];
  }
  const int total = block_sum<256>(s, wsum);
  if (t == 0) a.tile[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void covis_tile_scan_kernel(CovisArgs a, int tiles) {
  __shared__ int wsum[4];
  const int t = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < tiles; base += 256) {                // (uniform)
    const int b = base + t;
    const int v = b < tiles ? a.tile[b] : 0;
    int total;
    const int ex = block_excl_scan<256>(v, wsum, &total);
    if (b < tiles) a.tile[b] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(256) void covis_start_kernel(CovisArgs a) {
  __shared__ int wsum[4];
  constexpr int PER = CV_SCAN_TILE / 256;
  const int t = threadIdx.x, P = a.max_points + 1;
  const size_t base = (size_t)blockIdx.x * CV_SCAN_TILE + (size_t)t * PER;
  int v[PER];
  int s = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    v[k] = base + k < (size_t)P ? a.count[base + k] : 0;
    s += v[k];
  }
  int total;
  int run = a.tile[blockIdx.x] + block_excl_scan<256>(s, wsum, &total);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (base + k < (size_t)P) {
      a.start[base + k] = run;
      a.count[base + k] = 0;
    }
    run += v[k];
  }
}

__global__ __launch_bounds__(256) void covis_fill_kernel(CovisArgs a) {
  const int f = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < a.cap; i += 256) {
    const int p = a.packed[(size_t)f * a.cap + i];
    if (!cv_first(p)) continue;
    const int m = cv_id(p);
    const int at = a.start[m] + atomicAdd(a.count + m, 1);
    if (at < a.start[m + 1]) a.seg[at] = f;                      // (always: the segment was sized by the same marks)
  }
}

// w[f][.] into hist [size]: eight lanes share a row and walk the segment of its id
__device__ inline void covis_hist(const CovisArgs& a, int f, int* hist) {
  const int t = threadIdx.x, sub = t >> 3, l = t & 7;
  for (int g = t; g < a.size; g += 256) hist[g] = 0;
  __syncthreads();
  for (int i = sub; i < a.cap; i += 32) {
    const int m = cv_id(a.packed[(size_t)f * a.cap + i]);
    if (m < 0) continue;
    const int k1 = a.start[m + 1];
    for (int k = a.start[m] + l; k < k1; k += 8) {
      const int g = a.seg[k];
      if ((unsigned)g < (unsigned)a.size) atomicAdd(hist + g, 1);
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void covis_count_kernel(CovisArgs a) {
  __shared__ int hist[CV_MAX_FRAMES];
  __shared__ int wsum[4];
  const int f = blockIdx.x, t = threadIdx.x;
  covis_hist(a, f, hist);
  int c = 0;
  for (int g = t; g < a.size; g += 256) c += hist[g] > 0;
  const int total = block_sum<256>(c, wsum);
  if (t == 0) a.rowcnt[f] = total;
}

__global__ __launch_bounds__(256) void covis_rows_kernel(CovisArgs a) {
  __shared__ int wsum[4];
  const int t = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < a.size; base += 256) {               // (uniform)
    const int f = base + t;
    const int v = f < a.size ? a.rowcnt[f] : 0;
    int total;
    const int ex = block_excl_scan<256>(v, wsum, &total);
    if (f < a.size) a.row_ptr[f] = carry + ex;
    carry += total;
  }
  __syncthreads();
  const bool overflow = carry > a.max_edges;
  for (int f = t; f <= a.max_frames; f += 256) {
    if (overflow) a.row_ptr[f] = 0;
    else if (f >= a.size) a.row_ptr[f] = carry;
  }
  if (t == 0) {
    int32_t info[4];
    cv_info(info, carry, a.max_edges, a.acc[0], a.acc[1]);
    a.acc[2] = info[0];
    a.info[0] = info[0]; a.info[1] = info[1]; a.info[2] = info[2]; a.info[3] = info[3];
  }
}

__global__ __launch_bounds__(256) void covis_emit_kernel(CovisArgs a) {
  __shared__ int hist[CV_MAX_FRAMES];
  __shared__ int wsum[4];
  const int f = blockIdx.x, t = threadIdx.x;
  if (a.acc[2]) return;                                          // overflow: the graph stays empty (uniform)
  covis_hist(a, f, hist);
  int base = a.row_ptr[f];
  for (int g0 = 0; g0 < a.size; g0 += 256) {                     // (uniform)
    const int g = g0 + t;
    const int wt = g < a.size ? hist[g] : 0;
    int total;
    const int pos = base + block_compact<256>(wt > 0, wsum, &total);
    if (wt > 0 && pos < a.max_edges) {
      a.nbr[pos] = g;
      a.weight[pos] = wt;
    }
    base += total;
  }
}

}  // namespace

void launch_covis_segments(const CovisArgs& a, hipStream_t st) {
  const int tiles = (a.max_points + 1 + CV_SCAN_TILE - 1) / CV_SCAN_TILE;
  hipLaunchKernelGGL(covis_mark_kernel, dim3(a.size), dim3(256), 0, st, a);
  hipLaunchKernelGGL(covis_tile_sum_kernel, dim3(tiles), dim3(256), 0, st, a);
  hipLaunchKernelGGL(covis_tile_scan_kernel, dim3(1), dim3(256), 0, st, a, tiles);
  hipLaunchKernelGGL(covis_start_kernel, dim3(tiles), dim3(256), 0, st, a);
}

void launch_covis_build(const CovisArgs& a, hipStream_t st) {
  if (a.size > 0) {
    launch_covis_segments(a, st);
    hipLaunchKernelGGL(covis_fill_kernel, dim3(a.size), dim3(256), 0, st, a);
    hipLaunchKernelGGL(covis_count_kernel, dim3(a.size), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(covis_rows_kernel, dim3(1), dim3(256), 0, st, a);
  if (a.size > 0) hipLaunchKernelGGL(covis_emit_kernel, dim3(a.size), dim3(256), 0, st, a);
}

}  // namespace airfe
