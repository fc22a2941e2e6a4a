// airfe — batched loop detection on the device: MapRefiner::LoopDetection over a loaded map (src/map_refiner.cc:65-235) and the relative pose of
// RelativatePoseEstimation (:237-333).  Contract: include/airfe.h ("Stored queries against their predecessors", "Loop detection composite").  The rules
// are loopdet_core.h's, shared with the host statement; every sum is sequential in the order written, the file is compiled with -ffp-contract=off.
//   loopdet_init_kernel     the pose table to the identity, the right-image columns to -1
//   loopdet_qvec_kernel     (query)  the stored vector of frame d_qframe[q] -> row q of the query batch bowdb_query_kernel reads (an index outside the
//                           database: an empty vector)
//   loopdet_select_kernel   (query, 4 waves)  bowdb_select_kernel's job on the PREFIX 0 .. fq - 1: max_sharing and the threshold over the frames that were
//                           stored when the reference queried, the covisible frames found by binary search in row fq of the CSR, order-preserving
//                           compaction by ballot; frames from fq on are not read
//   loopdet_odom_kernel     (one workgroup)  the steps |pos[f] - pos[f - 1]| in parallel into LDS, ONE lane adds them up (sequential by contract)
//   loopdet_state_kernel    (query)  what the composite's later steps read of frame fq: its feature rows and count, position, max_dist, stored pose
//   loopdet_gather_kernel   (query)  the gates before the optimisation, then the winner's list entries whose candidate row has a map point -> constraints
//                           in list order, u_right from the stored frame's column
//   loopdet_finish_kernel   (query)  stage, ok, the relative pose
#include "bowgroup_core.h"
#include "common.h"
#include "kernels.h"
#include "loopdet_core.h"
#include "wg_prims.h"

namespace airfe {

namespace {

__global__ __launch_bounds__(256) void loopdet_init_kernel(double* pose, double* u_right, size_t n_pose, size_t n_ur) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  for (size_t k = i; k < n_pose; k += step) pose[k] = (k & 15) % 5 == 0 ? 1.0 : 0.0;
  for (size_t k = i; k < n_ur; k += step) u_right[k] = -1.0;
}

__global__ __launch_bounds__(256) void loopdet_qvec_kernel(LoopQvecArgs a) {
  const int q = blockIdx.x, t = threadIdx.x;
  const int fq = a.qframe[q];
  const bool in = fq >= 0 && fq < a.N;
  int n = in ? a.db_nw[fq] : 0;
  n = clamp_count(n, a.cap);
  if (t == 0) a.nw[q] = n;
  if (!in) return;
  const unsigned* si = a.db_ids + (size_t)fq * a.cap;
  const double* sv = a.db_vals + (size_t)fq * a.cap;
  for (int i = t; i < n; i += 256) {
    a.ids[(size_t)q * a.cap + i] = si[i];
    a.vals[(size_t)q * a.cap + i] = sv[i];
  }
}

__global__ __launch_bounds__(256) void loopdet_select_kernel(LoopSelectArgs a) {
  __shared__ int wsum[4];
  const int q = blockIdx.x, t = threadIdx.x;
  const int fq = a.qframe[q];
  const int limit = (fq >= 0 && fq < a.N) ? fq : 0;             // the frames that exist for this query: 0 .. limit - 1
  int* sh = a.sharing + (size_t)q * a.N;
  const double* sc = a.score + (size_t)q * a.N;
  int m = 0;
  for (int f = t; f < limit; f += 256) m = max(m, sh[f]);
  const int ms = block_max<256>(m, wsum);                       // over the PREFIX, before the filters (map_refiner.cc:104-107 on the database of :88-89)
  if (t == 0) a.max_sharing[q] = ms;
  const int thr = ld_threshold(ms, a.ratio, a.min_words);
  int base = 0;
  for (int f0 = 0; f0 < limit; f0 += 256) {                     // (uniform)
    const int f = f0 + t;
    bool keep = false;
    int s = 0;
    if (f < limit) {
      s = sh[f];
      keep = ld_candidate(s, thr, a.row_ptr != nullptr && ld_covisible(a.row_ptr, a.nbr, a.rows, fq, f));
    }
    int total;
    const int pos = base + block_compact<256>(keep, wsum, &total);
    if (keep && pos < a.ccap) {
      a.cand_frame[(size_t)q * a.ccap + pos] = f;
      a.cand_sharing[(size_t)q * a.ccap + pos] = s;
      a.cand_score[(size_t)q * a.ccap + pos] = sc[f];
    }
    base += total;
  }
  if (a.zero_tail)                                              // the caller's dense counts: a frame that does not exist shares nothing
    for (int f = limit + t; f < a.N; f += 256) sh[f] = 0;
  if (t == 0) a.ncand[q] = base;
}

__global__ __launch_bounds__(256) void loopdet_odom_kernel(const double* pos, int N, double* odom) {
  __shared__ double step[LD_MAX_FRAMES];
  const int t = threadIdx.x;
  for (int f = t; f < N; f += 256) step[f] = f > 0 ? ld_step(pos + 3 * (size_t)(f - 1), pos + 3 * (size_t)f) : 0.0;
  __syncthreads();
  if (t == 0) ld_prefix(step, N, step);                         // in place: entry f is read before it is written
  __syncthreads();
  for (int f = t; f < N; f += 256) odom[f] = step[f];
}

__global__ __launch_bounds__(256) void loopdet_state_kernel(LoopStateArgs a) {
  const int q = blockIdx.x, t = threadIdx.x;
  const int fq = a.qframe[q];
  const bool in = fq >= 0 && fq < a.N;
  int n = in ? a.db_n[fq] : 0;
  n = clamp_count(n, a.cap);
  if (t == 0) {
    a.qn[q] = n;
    a.max_dist[q] = in ? a.odom[fq] * a.distance_rate : 0.0;
  }
  if (t < 3) a.qpos[3 * (size_t)q + t] = in ? a.pos[3 * (size_t)fq + t] : 0.0;
  if (t < 16) a.Twc0[16 * (size_t)q + t] = in ? a.pose[16 * (size_t)fq + t] : (t % 5 == 0 ? 1.0 : 0.0);
  if (!in) return;
  const float* s = a.db_feat + (size_t)fq * a.cap * 259;
  float* d = a.qfeat + (size_t)q * a.cap * 259;
  for (int i = t; i < n * 259; i += 256) d[i] = s[i];
}

__global__ __launch_bounds__(256) void loopdet_gather_kernel(LoopGatherArgs g) {
  __shared__ int wsum[4];
  const int q = blockIdx.x, t = threadIdx.x;
  int m = g.nmatch[q];
  m = clamp_count(m, g.mcap);
  const int best = g.best[q];
  const int fq = g.qframe[q];
  int pre = ld_stage_before(g.ncand[q], g.gstatus[q], g.ngroups[q], best, g.N, m, g.min_matches);
  if (!pre && (fq < 0 || fq >= g.N)) pre = 1;                   // (cannot happen: such a query has no candidate; this is memory safety only)
  if (pre) m = 0;
  const int32_t* idx = g.idx + (size_t)q * g.mcap * 2;
  int* map = g.map + (size_t)q * g.mcap;
  double* X = g.X + (size_t)q * g.mcap * 3;
  double* obs = g.obs + (size_t)q * g.mcap * 3;
  int kept = 0;
  for (int base = 0; base < m; base += 256) {                   // (uniform)
    const int j = base + t;
    bool valid = false;
    double px[3] = {0.0, 0.0, 0.0}, po[3] = {0.0, 0.0, 0.0};
    if (j < m) {
      const int qi = idx[2 * j], ci = idx[2 * j + 1];
      if (qi >= 0 && qi < g.cap && ci >= 0 && ci < g.cap)       // the matcher's indices are in range; this is memory safety only
        valid = ld_constraint(g.xyz + ((size_t)best * g.cap + ci) * 3, g.feat + ((size_t)fq * g.cap + qi) * 259, g.u_right[(size_t)fq * g.cap + qi], px, po);
    }
    int total;
    const int s = kept + block_compact<256>(valid, wsum, &total);
    if (valid) {
      map[s] = j;
      X[3 * s] = px[0]; X[3 * s + 1] = px[1]; X[3 * s + 2] = px[2];
      obs[3 * s] = po[0]; obs[3 * s + 1] = po[1]; obs[3 * s + 2] = po[2];
    }
    kept += total;
  }
  if (t == 0) {
    g.n[q] = kept;
    g.n_opt[q] = (!pre && kept >= g.min_points) ? kept : 0;     // fewer than min_points (:301): none are handed over, the pose stays the stored one
    g.pre[q] = pre;
  }
}

__global__ __launch_bounds__(64) void loopdet_finish_kernel(LoopFinishArgs f) {
  const int q = blockIdx.x;
  if (threadIdx.x != 0) return;
  const int ncons = f.ncons[q], best = f.best[q];
  const int stage = ld_stage(f.pre[q], ncons, f.min_points, f.num[q], f.min_inliers);
  f.stage[q] = stage;
  f.ok[q] = stage == 0 ? 1 : 0;
  if (f.ncons_out) f.ncons_out[q] = ncons;
  if ((stage == 0 || stage == 5) && best >= 0 && best < f.N) ld_relative_pose(f.pose + 16 * (size_t)best, f.Twq + 16 * (size_t)q, f.Rlq + 9 * (size_t)q, f.tlq + 3 * (size_t)q);
  else ld_no_relative_pose(f.Rlq + 9 * (size_t)q, f.tlq + 3 * (size_t)q);
}

}  // namespace

void launch_loopdet_init(double* pose, double* u_right, int frames, int cap, hipStream_t st) {
  hipLaunchKernelGGL(loopdet_init_kernel, dim3(256), dim3(256), 0, st, pose, u_right, (size_t)frames * 16, (size_t)frames * cap);
}

void launch_loopdet_qvec(const LoopQvecArgs& a, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(loopdet_qvec_kernel, dim3(Q), dim3(256), 0, st, a);
}

void launch_loopdet_select(const LoopSelectArgs& a, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(loopdet_select_kernel, dim3(Q), dim3(256), 0, st, a);
}

void launch_loopdet_odom(const double* pos, int N, double* odom, hipStream_t st) {
  if (N < 1 || N > LD_MAX_FRAMES) return;
  hipLaunchKernelGGL(loopdet_odom_kernel, dim3(1), dim3(256), 0, st, pos, N, odom);
}

void launch_loopdet_state(const LoopStateArgs& a, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(loopdet_state_kernel, dim3(Q), dim3(256), 0, st, a);
}

void launch_loopdet_gather(const LoopGatherArgs& g, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(loopdet_gather_kernel, dim3(Q), dim3(256), 0, st, g);
}

void launch_loopdet_finish(const LoopFinishArgs& f, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(loopdet_finish_kernel, dim3(Q), dim3(64), 0, st, f);
}

}  // namespace airfe
