// airfe — workgroup primitives of the kernels: wave and workgroup reductions, the exclusive scan, the ordered compaction, the bitonic sort.  Device only;
// included after common.h.  THREADS is the workgroup size (1-D, a multiple of 64); `wsum` / `red` is the caller's LDS scratch of THREADS / 64 elements.
//
// THE BARRIER CONTRACT, the same for every block_* primitive:
//   1. All threads of the workgroup call the primitive, under uniform control flow.
//   2. The primitive's first barrier orders everything the caller did before the call (loads included) before anything the caller does after it:
//      a kernel may read a chunk, call, and write the same chunk in place; LDS the caller wrote before the call is visible to every thread after it.
//   3. The scratch is free again on return (the last barrier is behind the last read of it): the next call, of any primitive, may reuse it at once.
// So a scan, a compaction and a reduction are two barriers each (scratch written | read |), whatever THREADS; block_sort_asc opens with a barrier of its
// own and closes every stage with one, so the keys need no barrier in front of the call and are sorted and visible behind it.
// The wave_* primitives have no barrier and no LDS: 64 lanes, every lane gets the result.
#pragma once
#include "common.h"

namespace airfe {

__device__ __forceinline__ int wg_max2(int a, int b) { return max(a, b); }
__device__ __forceinline__ unsigned wg_max2(unsigned a, unsigned b) { return max(a, b); }
__device__ __forceinline__ float wg_max2(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int wg_min2(int a, int b) { return min(a, b); }
__device__ __forceinline__ unsigned wg_min2(unsigned a, unsigned b) { return min(a, b); }
__device__ __forceinline__ float wg_min2(float a, float b) { return fminf(a, b); }

// xor butterfly 32 .. 1 (int, unsigned, float): the order of a float sum is part of its bits
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = wg_max2(v, __shfl_xor(v, o));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = wg_min2(v, __shfl_xor(v, o));
  return v;
}

// one integer atomic per wave: the lanes with `yes` counted into *at (none when there is none)
__device__ __forceinline__ void wave_count_add(bool yes, int* at) {
  const int c = __popcll(__ballot(yes));
  if (c && (threadIdx.x & 63) == 0) atomicAdd(at, c);
}

// sum / max / min of one int per thread; every thread gets it
template <int THREADS>
__device__ __forceinline__ int block_sum(int v, int* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int k = 1; k < THREADS / 64; ++k) r += red[k];
  __syncthreads();
  return r;
}
template <int THREADS>
__device__ __forceinline__ int block_max(int v, int* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int k = 1; k < THREADS / 64; ++k) r = max(r, red[k]);
  __syncthreads();
  return r;
}
template <int THREADS>
__device__ __forceinline__ int block_min(int v, int* red) {
  v = wave_min(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int k = 1; k < THREADS / 64; ++k) r = min(r, red[k]);
  __syncthreads();
  return r;
}

// exclusive prefix sum of one T (int or unsigned) per thread in thread order; *total = the sum.  A shuffle scan inside each wave, the wave totals through LDS.
template <int THREADS, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* wsum, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(incl, o);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  T off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) {
    const T s = wsum[k];
    if (k < w) off += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return off + incl - v;
}

// exclusive prefix MAX in thread order: the largest v of the threads before this one, `none` for thread 0 (none <= every v)
template <int THREADS>
__device__ __forceinline__ int block_excl_scan_max(int v, int none, int* wmax) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o);
    if (lane >= o) incl = max(incl, u);
  }
  if (lane == 63) wmax[w] = incl;
  __syncthreads();
  int e = __shfl_up(incl, 1);
  if (lane == 0) e = none;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k)
    if (k < w) e = max(e, wmax[k]);
  __syncthreads();
  return e;
}

// ordered compaction: the number of threads with `keep` before this one in thread order; *total = all of them.  Ballot + popcount, no shuffle scan.
template <int THREADS>
__device__ __forceinline__ int block_compact(bool keep, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) wsum[w] = __popcll(bal);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) {
    const int s = wsum[k];
    if (k < w) off += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return off + __popcll(bal & ((1ull << lane) - 1ull));
}

// ascending bitonic sort of key[0 .. P) in LDS, P a power of two (smaller than THREADS is fine: the other threads only keep the barriers)
template <int THREADS, class T>
__device__ __forceinline__ void block_sort_asc(T* key, int P) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P; i += THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const T x = key[i], y = key[l];
          if ((x > y) == ((i & k) == 0)) { key[i] = y; key[l] = x; }
        }
      }
      __syncthreads();
    }
}

}  // namespace airfe
