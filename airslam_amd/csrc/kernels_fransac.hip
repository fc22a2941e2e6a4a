// airfe — the F-matrix RANSAC behind MatchingPoints(..., outlier_rejection = true) (src/point_matcher.cc:95-104) on B device match lists, in place.
// Contract: include/airfe.h ("F-matrix RANSAC"); per-sample arithmetic: fransac_core.h.  Three kernels on the caller's stream:
//   fransac_models_kernel  (chunk of 128 samples, pair): one lane draws + solves one sample (models in LDS), then the two waves score the models,
//                          lanes striding over the matches: RANSAC = inlier count (wave ballot), LMedS = median error (rank by shuffles; <= 14 matches)
//   fransac_scan_kernel    (pair): the sequential rule over the scores in sample order, as a block scan: the best count before sample s fixes
//                          niters(s); the search stops at the first s >= niters(s); the winner is the first model with the largest count before it
//   fransac_compact_kernel (pair): the winner re-solved (same code, same bits), its mask, an order-preserving compaction of idx / score / nmatch
// The models kernel runs twice: samples [0, 256), then [256, 1000) only for pairs whose niters bound still reaches a chunk.
#include "common.h"
#include "kernels.h"
#include "fransac_core.h"
#include "wg_prims.h"

namespace airfe {

namespace {

constexpr int FR_CHUNK = 128;         // samples per models workgroup (one per lane of its two waves)
constexpr int FR_FIRST = 256;         // samples of the first slice

// truncated (cv::Point = Point_<int> built from the floats: toward zero) coordinates of pair b's n matches -> LDS [n][4]
__device__ void load_points(const FransacArgs& a, int b, int n, float* xy) {
  const float* f0 = a.f0 + (size_t)b * a.cap * 259;
  const float* f1 = a.f1 + (size_t)b * a.cap * 259;
  const int32_t* idx = a.idx + (size_t)b * a.mcap * 2;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    int q = idx[2 * i], t = idx[2 * i + 1];
    q = q < 0 ? 0 : (q >= a.cap ? a.cap - 1 : q);        // memory safety only: the matcher's indices are in range
    t = t < 0 ? 0 : (t >= a.cap ? a.cap - 1 : t);
    xy[4 * i + 0] = truncf(f0[(size_t)q * 259 + 1]);
    xy[4 * i + 1] = truncf(f0[(size_t)q * 259 + 2]);
    xy[4 * i + 2] = truncf(f1[(size_t)t * 259 + 1]);
    xy[4 * i + 3] = truncf(f1[(size_t)t * 259 + 2]);
  }
}

__device__ __forceinline__ int pair_n(const FransacArgs& a, int b) {
  return clamp_count(a.nmatch[b], a.mcap);
}

__global__ __launch_bounds__(FR_CHUNK) void fransac_models_kernel(FransacArgs a, int chunk0) {
  __shared__ float xy[FR_MAX_MATCHES * 4];
  __shared__ double sF[FR_CHUNK * 3][9];
  __shared__ int snm[FR_CHUNK];
  const int b = blockIdx.y, chunk = chunk0 + blockIdx.x;
  const int n = pair_n(a, b);
  if (n < 9) return;
  const bool lmeds = n < FR_MIN_RANSAC;
  const int total = lmeds ? FR_LMEDS_ITERS : FR_RANSAC_ITERS, s0 = chunk * FR_CHUNK;
  if (s0 >= total) return;
  if (chunk0 > 0) {                                          // later slice: only where the first slice's scan left the search open this far
    const int* st = a.state + 4 * b;
    if (st[1] || s0 >= st[0]) return;
  }
  load_points(a, b, n, xy);
  __syncthreads();
  const int t = threadIdx.x, s = s0 + t;
  int m = 0;
  if (s < total) {
    double X[7][4];
    if (fr_sample(xy, n, s, X)) m = fr_solve7(X, &sF[3 * t]);
  }
  snm[t] = m;
  int* out = a.scores + ((size_t)b * FR_RANSAC_ITERS + s) * 3;
  if (s < total)
    for (int r = m; r < 3; ++r) out[r] = -1;                 // no model: never selected (as int: <= 6; as uint: above +inf's bits)
  __syncthreads();
  const int lane = t & 63, w = t >> 6;
  for (int k = w; k < FR_CHUNK * 3; k += FR_CHUNK / 64) {
    const int ls = k / 3, r = k - 3 * ls;
    if (s0 + ls >= total || r >= snm[ls]) continue;          // wave-uniform
    const double* f = sF[k];
    int val;
    if (!lmeds) {
      int cnt = 0;
      for (int i = lane; i < n; i += 64) {
        const float e = fr_error(f, xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3]);
        cnt += __popcll(__ballot(e <= FR_THRESH2));
      }
      val = cnt;                                             // (lane 0 took part in every ballot)
    } else {
      // n <= 14: lane i holds error i; the median is the element of rank n / 2 (ties broken by index)
      const float e = lane < n ? fr_error(f, xy[4 * lane], xy[4 * lane + 1], xy[4 * lane + 2], xy[4 * lane + 3]) : INFINITY;
      int rank = 0;
      for (int j = 0; j < FR_MIN_RANSAC - 1; ++j) {
        const float ej = __shfl(e, j, 64);
        rank += (j < n) && (ej < e || (ej == e && j < lane));
      }
      const unsigned long long hit = __ballot(lane < n && rank == n / 2);
      const float med = __shfl(e, (int)__ffsll((long long)hit) - 1, 64);
      val = (int)__float_as_uint(med);
    }
    if (lane == 0) a.scores[((size_t)b * FR_RANSAC_ITERS + s0 + ls) * 3 + r] = val;
  }
}

__global__ __launch_bounds__(1024) void fransac_scan_kernel(FransacArgs a, int final_pass) {
  __shared__ int red[16], wmax[16], bcast[2];
  const int b = blockIdx.x, t = threadIdx.x;
  int* st = a.state + 4 * b;
  const int n = pair_n(a, b);
  if (n < 9) {
    if (t == 0) st[0] = 0, st[1] = 1, st[2] = -2;           // the gate: the list stays as it is
    return;
  }
  if (final_pass && st[1]) return;                            // decided by the first slice
  const int* sc = a.scores + (size_t)b * FR_RANSAC_ITERS * 3;
  if (n < FR_MIN_RANSAC) {                                    // LMedS: every one of its 300 samples, smallest median, first wins
    if (!final_pass) {
      if (t == 0) st[0] = FR_LMEDS_ITERS, st[1] = 0, st[2] = -1;
      return;
    }
    int v = 0x7FFFFFFF;                                       // float bits of a finite median (non-negative); +inf / no model: never
    if (t < FR_LMEDS_ITERS)
      for (int r = 0; r < 3; ++r) {
        const unsigned u = (unsigned)sc[3 * t + r];
        if (u < 0x7F800000u) v = min(v, (int)u);
      }
    const int mn = block_min<1024>(v, red);
    int pos = 0x7FFFFFFF;
    if (t < FR_LMEDS_ITERS && mn != 0x7FFFFFFF && v == mn)
      for (int r = 2; r >= 0; --r)
        if (sc[3 * t + r] == mn) pos = 3 * t + r;
    const int sel = block_min<1024>(pos, red);
    if (t == 0) st[0] = FR_LMEDS_ITERS, st[1] = 1, st[2] = mn == 0x7FFFFFFF ? -1 : sel;
    return;
  }
  const int limit = final_pass ? FR_RANSAC_ITERS : FR_FIRST;
  int v = -1;
  if (t < limit)
    for (int r = 0; r < 3; ++r) v = max(v, sc[3 * t + r]);
  const int E = block_excl_scan_max<1024>(v, -1, wmax);      // E(t) = best count over the samples before t
  const int nb = E > 6 ? fr_update_niters(n, E) : FR_RANSAC_ITERS;      // niters when sample t is reached
  const bool pred = t <= limit && t >= nb;
  const int stop = block_min<1024>(pred ? t : 0x7FFFFFFF, red);
  if (stop == 0x7FFFFFFF) {                                   // first slice: still open; the bound for the next slice
    if (t == limit) st[0] = nb, st[1] = 0, st[2] = -1;
    return;
  }
  if (t == stop) bcast[0] = E;
  __syncthreads();
  const int best = bcast[0];
  int pos = 0x7FFFFFFF;
  if (best > 6 && t < stop)
    for (int r = 2; r >= 0; --r)
      if (sc[3 * t + r] == best) pos = 3 * t + r;
  const int sel = block_min<1024>(pos, red);
  if (t == 0) st[0] = stop, st[1] = 1, st[2] = best > 6 ? sel : -1;
}

__global__ __launch_bounds__(256) void fransac_compact_kernel(FransacArgs a) {
  __shared__ float xy[FR_MAX_MATCHES * 4];
  __shared__ double sF[3][9];
  __shared__ int wsum[4], sh[2];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int n = pair_n(a, b);
  const int* st = a.state + 4 * b;
  const int sel = n < 9 ? -2 : st[2];
  double* F = a.F ? a.F + 9 * (size_t)b : nullptr;
  if (sel < 0) {
    if (F && t < 9) F[t] = 0.0;
    if (sel == -1 && t == 0) a.nmatch[b] = 0;                 // no model: nothing is kept
    return;
  }
  load_points(a, b, n, xy);
  __syncthreads();
  const int s = sel / 3, r = sel - 3 * s;
  if (t == 0) {
    double X[7][4];
    int m = 0;
    if (fr_sample(xy, n, s, X)) m = fr_solve7(X, sF);
    sh[0] = m > r;
  }
  __syncthreads();
  if (!sh[0]) {                                               // cannot happen (the scan picked an existing model); keep the list untouched
    if (F && t < 9) F[t] = 0.0;
    return;
  }
  const double* f = sF[r];
  const bool lmeds = n < FR_MIN_RANSAC;
  const float thr = lmeds ? fr_lmeds_thresh(n, __uint_as_float((unsigned)a.scores[((size_t)b * FR_RANSAC_ITERS) * 3 + sel])) : FR_THRESH2;
  if (F && t < 9) F[t] = f[t];
  if (lmeds) {                                                // fewer than 7 inliers: LMedS reports failure, nothing is kept
    if (w == 0) {
      const bool in = lane < n && fr_error(f, xy[4 * lane], xy[4 * lane + 1], xy[4 * lane + 2], xy[4 * lane + 3]) <= thr;
      const int c = __popcll(__ballot(in));
      if (lane == 0) sh[1] = c;
    }
    __syncthreads();
    if (sh[1] < 7) {
      if (t == 0) a.nmatch[b] = 0;
      return;
    }
  }
  int32_t* idx = a.idx + (size_t)b * a.mcap * 2;
  float* score = a.score + (size_t)b * a.mcap;
  int kept = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + t;
    int2 id = make_int2(0, 0);
    float sv = 0.f;
    bool in = false;
    if (i < n) {
      id = make_int2(idx[2 * i], idx[2 * i + 1]);
      sv = score[i];
      in = fr_error(f, xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3]) <= thr;
    }
    int total;                                                // in place: every element of this chunk is read before any is written, by the barrier
    const int o = kept + block_compact<256>(in, wsum, &total);      // contract of wg_prims.h (rule 2)
    if (in) {
      idx[2 * o] = id.x; idx[2 * o + 1] = id.y;
      score[o] = sv;
    }
    kept += total;
  }
  if (t == 0) a.nmatch[b] = kept;
}

}  // namespace

void launch_fransac(const FransacArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(fransac_models_kernel, dim3(FR_FIRST / FR_CHUNK, B), dim3(FR_CHUNK), 0, st, a, 0);
  hipLaunchKernelGGL(fransac_scan_kernel, dim3(B), dim3(1024), 0, st, a, 0);
  hipLaunchKernelGGL(fransac_models_kernel, dim3((FR_RANSAC_ITERS - FR_FIRST + FR_CHUNK - 1) / FR_CHUNK, B), dim3(FR_CHUNK), 0, st, a, FR_FIRST / FR_CHUNK);
  hipLaunchKernelGGL(fransac_scan_kernel, dim3(B), dim3(1024), 0, st, a, 1);
  hipLaunchKernelGGL(fransac_compact_kernel, dim3(B), dim3(256), 0, st, a);
}

}  // namespace airfe
