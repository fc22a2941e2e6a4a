// airfe — relocalisation to the pose on the device: the GROUPING between the BoW scores and the candidates (src/map_user.cc:177-270, 331, 347-363;
// src/map_refiner.cc:132-214) and the composite's glue around the matcher, the PnP RANSAC and the frame optimisation (map_user.cc:377-460).
// Contract: include/airfe.h ("Grouping", "Relocalisation composite").  The per-candidate, per-group and ranking routines are bowgroup_core.h's, shared
// with the host statement; every sum is sequential in the order written, the file is compiled with -ffp-contract=off.
//   bowgroup_kernel       (query, 4 waves)  the candidate list in LDS; one lane per candidate (striding) walks its covisibility row, neighbours found by
//                         binary search in the ascending frame list; ONE lane runs the replacement rule over group_of[deputy slot] in list order (it is
//                         sequential by contract); the re-sum / distance filter, the 0.5 filter and the junction term are parallel over the stored groups
//                         (membership is walked again, not stored); K selection passes rank them
//   reloc_gather_kernel   (query)  the gates before PnP, then the winner's list entries whose candidate row has a map point -> PnP correspondences and
//                         frame-optimisation constraints, in list order, indirected through d_best[q] into the database's point table
//   reloc_finish_kernel   the final gate: stage and ok per query
#include "bowgroup_core.h"
#include "common.h"
#include "kernels.h"
#include "wg_prims.h"

namespace airfe {

namespace {

__global__ __launch_bounds__(256) void bowgroup_kernel(BowGroupArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int C = a.ccap;
  double* score = reinterpret_cast<double*>(smem);              // [C] the candidates' scores
  double* gscore = score + C;                                   // [C] per candidate: its group's score
  double* fin = gscore + C;                                     // [C] per deputy slot: the stored group's final score
  int* frame = reinterpret_cast<int*>(fin + C);                 // [C] the candidates' frames, ascending
  int* deputy = frame + C;                                      // [C] per candidate: its deputy's slot
  int* group_of = deputy + C;                                   // [C] per deputy slot: the candidate whose group is stored (-1: none / dropped)
  __shared__ double rs[256];
  __shared__ int rp[256], ri[4];
  __shared__ double s_best;
  const int q = blockIdx.x, t = threadIdx.x;
  int32_t* out_frame = a.group_frame + (size_t)q * a.K;
  double* out_score = a.group_score + (size_t)q * a.K;
  const int nc = a.ncand[q];
  if (nc > C || nc <= 0) {                                      // (uniform) an incomplete list is not grouped; an empty one has no group
    if (t < a.K) { out_frame[t] = -1; out_score[t] = 0.0; }
    if (t == 0) { a.ngroups[q] = 0; a.status[q] = nc > C ? BG_OVERFLOW : BG_NO_GROUP; }
    return;
  }
  const int n = nc;
  for (int i = t; i < n; i += 256) {
    frame[i] = a.cand_frame[(size_t)q * C + i];
    score[i] = a.cand_score[(size_t)q * C + i];
    group_of[i] = -1;
  }
  __syncthreads();
  for (int i = t; i < n; i += 256) {
    double g;
    int d;
    bg_candidate(frame, score, n, a.row_ptr, a.nbr, a.weight, a.rows, i, &g, &d);
    gscore[i] = g;
    deputy[i] = d;
  }
  __syncthreads();
  if (t == 0) s_best = bg_replace(gscore, deputy, n, group_of);
  __syncthreads();
  const double best_group = s_best;
  if (best_group < 0) {                                         // (uniform)
    if (t < a.K) { out_frame[t] = -1; out_score[t] = 0.0; }
    if (t == 0) { a.ngroups[q] = 0; a.status[q] = BG_NO_GROUP; }
    return;
  }
  int cnt = 0;
  double mx = 0.0;
  for (int d = t; d < n; d += 256) {
    const int g = group_of[d];
    if (g < 0) continue;
    if (a.mode == BG_MODE_RELOC) {
      const double v = bg_resum(frame, score, n, a.row_ptr, a.nbr, a.weight, a.rows, g);
      fin[d] = v;
      if (mx < v) mx = v;
    } else {
      fin[d] = gscore[g];
      const int f = frame[d];
      if (f >= 0 && f < a.pos_rows && bg_far(a.qpos + 3 * (size_t)q, a.pos + 3 * (size_t)f, a.max_dist[q])) { group_of[d] = -1; continue; }
    }
    ++cnt;
  }
  rs[t] = mx;
  const int stored = block_sum<256>(cnt, ri);                   // (its first barrier orders rs as well)
  for (int d = 128; d > 0; d >>= 1) {
    if (t < d && rs[t] < rs[t + d]) rs[t] = rs[t + d];
    __syncthreads();
  }
  const double best = a.mode == BG_MODE_RELOC ? rs[0] : best_group;
  __syncthreads();
  const double thr = best * 0.5;
  const double* extra = a.mode == BG_MODE_RELOC && a.extra ? a.extra + (size_t)q * a.n_extra : nullptr;
  cnt = 0;
  for (int d = t; d < n; d += 256) {
    if (group_of[d] < 0) continue;
    if (stored > 3 && fin[d] < thr) { group_of[d] = -1; continue; }
    const int f = frame[d];
    if (extra && f >= 0 && f < a.n_extra) fin[d] += extra[f];
    ++cnt;
  }
  const int left = block_sum<256>(cnt, ri);
  if (t == 0) { a.ngroups[q] = left; a.status[q] = BG_OK; }
  double ps = 0.0;
  int pp = -1;
  for (int r = 0; r < a.K; ++r) {                               // (uniform: ps / pp come from LDS)
    double bs = 0.0;
    int bp = -1;
    for (int d = t; d < n; d += 256)
      if (group_of[d] >= 0 && (r == 0 || bg_behind(fin[d], d, ps, pp)) && bg_before(fin[d], d, bs, bp)) { bs = fin[d]; bp = d; }
    rs[t] = bs;
    rp[t] = bp;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {                         // the ranking is a strict total order: any reduction tree finds the same group
      if (t < d && rp[t + d] >= 0 && bg_before(rs[t + d], rp[t + d], rs[t], rp[t])) { rs[t] = rs[t + d]; rp[t] = rp[t + d]; }
      __syncthreads();
    }
    ps = rs[0];
    pp = rp[0];
    __syncthreads();
    if (pp < 0) {                                               // fewer than K groups: -1 padding
      if (t >= r && t < a.K) { out_frame[t] = -1; out_score[t] = 0.0; }
      break;
    }
    if (t == 0) { out_frame[r] = frame[pp]; out_score[r] = ps; }
  }
}

__global__ __launch_bounds__(256) void reloc_gather_kernel(RelocGatherArgs g) {
  __shared__ int wsum[4];
  const int q = blockIdx.x, t = threadIdx.x;
  int m = clamp_count(g.nmatch[q], g.mcap);
  const int best = g.best[q];
  int pre = 0;                                                  // the gates of map_user.cc:139 / 158, :219, :377
  if (g.ncand[q] <= 0) pre = 1;
  else if (g.gstatus[q] != BG_OK || g.ngroups[q] <= 0) pre = 2;
  else if (best < 0 || best >= g.N || m < g.min_inlier) pre = 3;
  if (pre) m = 0;
  const int32_t* idx = g.idx + (size_t)q * g.mcap * 2;
  float* obj = g.obj + (size_t)q * g.mcap * 3;
  float* img = g.img + (size_t)q * g.mcap * 2;
  int* map = g.map + (size_t)q * g.mcap;
  double* X = g.X + (size_t)q * g.mcap * 3;
  double* obs = g.obs + (size_t)q * g.mcap * 3;
  int kept = 0;
  for (int base = 0; base < m; base += 256) {
    const int j = base + t;
    bool valid = false;
    double px = 0.0, py = 0.0, pz = 0.0;
    float u = 0.f, v = 0.f;
    if (j < m) {
      const int qi = idx[2 * j], ci = idx[2 * j + 1];
      if (qi >= 0 && qi < g.cap && ci >= 0 && ci < g.cap) {     // the matcher's indices are in range; this is memory safety only
        const double* p = g.xyz + ((size_t)best * g.cap + ci) * 3;
        px = p[0]; py = p[1]; pz = p[2];
        valid = !is_nan(px);
        const float* f = g.qfeat + ((size_t)q * g.cap + qi) * 259;
        u = f[1]; v = f[2];
      }
    }
    int total;
    const int s = kept + block_compact<256>(valid, wsum, &total);
    if (valid) {
      obj[3 * s] = (float)px; obj[3 * s + 1] = (float)py; obj[3 * s + 2] = (float)pz;      // cv::Point3f
      img[2 * s] = u; img[2 * s + 1] = v;
      map[s] = j;
      X[3 * s] = px; X[3 * s + 1] = py; X[3 * s + 2] = pz;
      obs[3 * s] = (double)u; obs[3 * s + 1] = (double)v; obs[3 * s + 2] = -1.0;           // the query frame has no right image: every edge mono
    }
    kept += total;
  }
  if (t == 0) {
    if (!pre && g.refine && kept < g.min_inlier) pre = 4;       // map_user.cc:448, behind PnP: the pose stays PnP's
    g.n[q] = kept;
    g.n_opt[q] = (g.refine && !pre) ? kept : 0;
    g.pre[q] = pre;
  }
}

__global__ __launch_bounds__(256) void reloc_finish_kernel(RelocFinishArgs f, int Q) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const int pre = f.pre[q];
  const int stage = pre ? pre : (f.num[q] < f.min_inlier ? 5 : 0);                          // map_user.cc:460
  f.stage[q] = stage;
  f.ok[q] = stage == 0 ? 1 : 0;
  if (f.pnp_count_out) f.pnp_count_out[q] = f.pnp_count[q];
}

}  // namespace

size_t bowgroup_lds(int ccap) { return (size_t)ccap * 36; }

int launch_bowgroup(const BowGroupArgs& a, int Q, hipStream_t st) {
  if (Q < 1) return 0;
  const size_t lds = bowgroup_lds(a.ccap);
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(bowgroup_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(bowgroup_kernel, dim3(Q), dim3(256), lds, st, a);
  return 0;
}

void launch_reloc_gather(const RelocGatherArgs& g, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(reloc_gather_kernel, dim3(Q), dim3(256), 0, st, g);
}

void launch_reloc_finish(const RelocFinishArgs& f, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(reloc_finish_kernel, dim3((Q + 255) / 256), dim3(256), 0, st, f, Q);
}

}  // namespace airfe
