// airfe — pose-only frame optimisation (FrameOptimization of tracking, src/g2o_optimization/g2o_optimization.cc:446-898 with one free pose and point
// edges only) on B device problems.  Contract: include/airfe.h ("Frame optimisation"); arithmetic: poseopt_core.h.
//   poseopt_kernel         (problem): ONE wave does the three rounds in one launch.  The constraints sit in LDS as six arrays (conflict-free: lane l
//                          reads element l of each); lane l owns partial l of H, b and chi in registers over the constraints l, l + 64, ...; the 64
//                          partials go through LDS and lanes 0..27 add one column each in lane order; lane 0 does the 6 x 6 solve and the
//                          Levenberg-Marquardt bookkeeping on the state in LDS (a single wave: the barriers around it cost next to nothing).
//   poseopt_gather_kernel  (problem): the composite's glue — the seed (PnP pose or the last tracked pose) and the constraints of the list entries
//                          the PnP gather kept, in its order
// The chain of trials is serial: the kernel's time is latency (LDS round trips of the solve, the dependent adds of the lane-order sums), not fp64 rate.
#include "common.h"
#include "kernels.h"
#include "poseopt_core.h"
#include "wg_prims.h"

namespace airfe {

namespace {

constexpr int PO_PART = 29;           // row stride of the partials in LDS (odd: lanes 0..27 read a row without conflicts, writes spread over the banks)

__global__ __launch_bounds__(PO_LANES) void poseopt_kernel(PoseoptArgs a) {
  __shared__ double cons[6 * PO_MAX_POINTS];
  __shared__ double part[PO_LANES * PO_PART];
  __shared__ double tot[28], S[PO_SIZE], hin[36];
  __shared__ uint8_t lvl[PO_MAX_POINTS];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = clamp_count(a.n[b], a.ncap);
  const double* gX = a.X + (size_t)b * a.ncap * 3;
  const double* gO = a.obs + (size_t)b * a.ncap * 3;
  for (int i = t; i < n; i += PO_LANES) {
    for (int k = 0; k < 3; ++k) { PO_C(cons, k, i) = gX[3 * i + k]; PO_C(cons, 3 + k, i) = gO[3 * i + k]; }
    lvl[i] = 0;
  }
  const double* Twc0 = a.Twc0 + 16 * (size_t)b;
  if (t < 16) hin[t] = Twc0[t];
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) hin[16 + k] = a.cam[k];
#pragma unroll
    for (int k = 0; k < 2; ++k) hin[21 + k] = a.thr[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) hin[23 + k] = a.Tcb[k];
  }
  __syncthreads();
  if (t == 0) {
    po_init(S, hin, a.has_tcb ? hin + 23 : nullptr, hin + 16, hin + 21);
    po_round_start(S);
  }
  __syncthreads();
  int outliers = 0;
  for (int round = 0; round < PO_ROUNDS && n > 0; ++round) {
    if (t == 0) po_round_start(S);
    __syncthreads();
    for (int it = 0; it < PO_ITERS; ++it) {
      double acc[28];
#pragma unroll
      for (int k = 0; k < 28; ++k) acc[k] = 0.0;
      for (int i = t; i < n; i += PO_LANES)
        if (!lvl[i]) po_edge_full(S + PO_CUR, S, cons, i, acc);
#pragma unroll
      for (int k = 0; k < 28; ++k) part[t * PO_PART + k] = acc[k];
      __syncthreads();
      if (t < 28) tot[t] = po_sum_lanes(part + t, PO_PART);
      __syncthreads();
      if (t == 0) po_iter_begin(S, tot, it);
      __syncthreads();
      while (S[PO_NEXT] == 0.0) {                                 // wave-uniform: S is in LDS
        if (t == 0) po_propose(S);
        __syncthreads();
        double c = 0.0;
        for (int i = t; i < n; i += PO_LANES)
          if (!lvl[i]) c = c + po_edge_chi(S + PO_TRY, S, cons, i);
        part[t] = c;
        __syncthreads();
        if (t == 0) po_judge(S, po_sum_lanes(part, 1));
        __syncthreads();
      }
      if (S[PO_STOP] != 0.0) break;
    }
    int out = 0;
    for (int i = t; i < n; i += PO_LANES) {
      const bool o = po_outlier(S + PO_CUR, S, cons, i);
      lvl[i] = o ? 1 : 0;
      out += o ? 1 : 0;
    }
    outliers = wave_sum(out);
    __syncthreads();
    if (n < PO_MIN_EDGES) break;
  }
  const bool good = n > 0 && po_finite12(S + PO_WB);
  const int num = good ? n - outliers : 0;
  // the composite keeps the seed unless more than lost_num_match constraints are inliers (map_builder.cc:397)
  const bool take = good && (a.lost < 0 || num > a.lost);
  __syncthreads();
  if (t == 0) {
    if (take) po_twc(S, hin);                                     // else hin[0..15] still holds the start pose
    else po_round_start(S);                                       // and Rt is the start pose's Rcw, tcw
  }
  __syncthreads();
  if (t < 16) a.Twc[16 * (size_t)b + t] = hin[t];
  if (a.Rt && t < 12) a.Rt[12 * (size_t)b + t] = canon_nan(S[PO_CUR + t]);
  uint8_t* mask = a.inlier + (size_t)b * a.mcap;
  if (a.map) {
    const int* map = a.map + (size_t)b * a.ncap;
    for (int i = t; i < a.mcap; i += PO_LANES) mask[i] = 0;
    __syncthreads();
    for (int i = t; i < n; i += PO_LANES) mask[map[i]] = (good && !lvl[i]) ? 1 : 0;
  } else {
    for (int i = t; i < a.mcap; i += PO_LANES) mask[i] = (i < n && good && !lvl[i]) ? 1 : 0;
  }
  if (t == 0) {
    a.num[b] = num;
    if (a.ok) a.ok[b] = (good && num > a.lost) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void poseopt_gather_kernel(PoseoptGatherArgs g) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = clamp_count(g.n[b], g.ncap);
  const int* map = g.map + (size_t)b * g.ncap;
  const int32_t* tidx = g.tidx + (size_t)b * g.mcap * 2;
  double* X = g.X + (size_t)b * g.ncap * 3;
  double* obs = g.obs + (size_t)b * g.ncap * 3;
  for (int q = t; q < n; q += 256) {
    const int j = map[q];                                        // (the PnP gather kept only entries whose indices are in range)
    const int r = tidx[2 * j], c = tidx[2 * j + 1];
    const double* p = g.xyz + ((size_t)b * g.capK + r) * 3;
    const float* f = g.feat + ((size_t)b * g.cap + c) * 259;
    X[3 * q] = p[0]; X[3 * q + 1] = p[1]; X[3 * q + 2] = p[2];
    obs[3 * q] = (double)f[1]; obs[3 * q + 1] = (double)f[2];
    obs[3 * q + 2] = g.u_right ? g.u_right[(size_t)b * g.cap + c] : -1.0;
  }
  if (t < 16) {
    const double* Tp = g.Twc_pnp + 16 * (size_t)b;
    const double* Tl = g.Twc_last ? g.Twc_last + 16 * (size_t)b : nullptr;
    const double last = Tl ? Tl[t] : ((t % 5) == 0 ? 1.0 : 0.0);
    const bool use_last = po_use_last(Tp, g.pnp_count[b], Tl ? Tl[3] : 0.0, Tl ? Tl[7] : 0.0, Tl ? Tl[11] : 0.0, g.lost);
    g.Twc0[16 * (size_t)b + t] = use_last ? last : Tp[t];
  }
}

}  // namespace

void launch_poseopt(const PoseoptArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(poseopt_kernel, dim3(B), dim3(PO_LANES), 0, st, a);
}
void launch_poseopt_gather(const PoseoptGatherArgs& g, int B, hipStream_t st) {
  hipLaunchKernelGGL(poseopt_gather_kernel, dim3(B), dim3(256), 0, st, g);
}

}  // namespace airfe
