// airfe — PnP RANSAC of SolvePnPWithCV (src/g2o_optimization/g2o_optimization.cc:1085-1134) on B device problems, and the stereo back-projection that
// feeds it (src/frame.cc:141-172, src/camera.cc:275-280).  Contract: include/airfe.h ("PnP RANSAC", "Stereo points"); arithmetic: pnp_core.h.
//   pnp_models_kernel  (chunk of 4 samples, problem): one lane draws + solves one sample with its EPnP workspace in LDS, then the wave scores the
//                      chunk's models, lanes striding over the correspondences (ballot count)
//   pnp_refine_kernel  (problem): the sequential rule over the 100 scores (one lane: it is 100 steps), the winner's mask, Levenberg-Marquardt on its
//                      inliers (lanes accumulate J^T J, J^T r in a fixed order; one lane solves the 6 x 6 system), the pose, the mask
//   pnp_gather_kernel  (problem): the composite's correspondences = temporal list entries whose keyframe point exists, in list order
//   pnp_stereo_kernel  (frame): the band + parallax test per stereo list entry (the last passing entry per left keypoint wins), the back-projection
// No kernel indexes a per-lane array with a runtime value: every array of pnp_core.h is reached through a pointer into LDS.
#include "common.h"
#include "kernels.h"
#include "pnp_core.h"
#include "wg_prims.h"

namespace airfe {

namespace {

constexpr int PNP_SPB = 4;            // samples per models workgroup (5.2 KB of LDS each); one lane solves a sample serially, ~1.1 ms: that latency is the kernel's time
constexpr int PNP_CHUNKS = (PNP_MAX_ITERS + PNP_SPB - 1) / PNP_SPB;

__global__ __launch_bounds__(64) void pnp_models_kernel(PnpArgs a) {
  __shared__ double ws[PNP_SPB][PNP_WS];
  __shared__ int ids[PNP_SPB][5];
  __shared__ int ok[PNP_SPB];
  __shared__ double sK[4];
  const int b = blockIdx.y, t = threadIdx.x, s0 = blockIdx.x * PNP_SPB;
  const int n = clamp_count(a.n[b], a.ncap);
  int* sc = a.scores + (size_t)b * PNP_MAX_ITERS;
  if (n < PNP_MIN_POINTS) {
    if (t < PNP_SPB && s0 + t < PNP_MAX_ITERS) sc[s0 + t] = -1;
    return;
  }
  if (t == 0) { sK[0] = a.fx; sK[1] = a.fy; sK[2] = a.cx; sK[3] = a.cy; }
  __syncthreads();
  const float* obj = a.obj + (size_t)b * a.ncap * 3;
  const float* img = a.img + (size_t)b * a.ncap * 2;
  double* models = a.models + (size_t)b * PNP_MAX_ITERS * 12;
  if (t < PNP_SPB) {
    const int s = s0 + t;
    bool m = false;
    if (s < PNP_MAX_ITERS) {
      m = pnp_solve_sample(obj, img, n, s, sK, ids[t], ws[t]);
      if (m)
        for (int k = 0; k < 12; ++k) models[12 * s + k] = ws[t][PW_BEST + k];
    }
    ok[t] = m;
  }
  __syncthreads();
  for (int k = 0; k < PNP_SPB; ++k) {
    const int s = s0 + k;
    if (s >= PNP_MAX_ITERS) break;
    if (!ok[k]) {                                              // wave-uniform
      if (t == 0) sc[s] = -1;
      continue;
    }
    const double* M = ws[k] + PW_BEST;
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + t;
      const bool in = i < n && pnp_error(M, obj[3 * i], obj[3 * i + 1], obj[3 * i + 2], img[2 * i], img[2 * i + 1], sK) <= PNP_THRESH2;
      cnt += __popcll(__ballot(in));
    }
    if (t == 0) sc[s] = cnt;
  }
}

// the refinement's sums at pose P over the masked points: lane l adds the points l, l + 64, ... in order, then lane k < 28 adds the 64 partials
__device__ void lm_accumulate(const double* P, const float* obj, const float* img, const uint8_t* msk, int n, const double* K, double (*part)[28],
                              double (*J)[12], double (*o)[28], double* tot) {
  const int t = threadIdx.x;
  for (int k = 0; k < 28; ++k) part[t][k] = 0.0;
  for (int i = t; i < n; i += PNP_LM_LANES) {
    if (!msk[i]) continue;
    pnp_lm_point(P, (double)obj[3 * i], (double)obj[3 * i + 1], (double)obj[3 * i + 2], (double)img[2 * i], (double)img[2 * i + 1], K, J[t], o[t]);
    for (int k = 0; k < 28; ++k) part[t][k] = part[t][k] + o[t][k];
  }
  __syncthreads();
  if (t < 28) {
    double s = 0.0;
    for (int l = 0; l < PNP_LM_LANES; ++l) s = s + part[l][t];
    tot[t] = s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(PNP_LM_LANES) void pnp_refine_kernel(PnpArgs a) {
  __shared__ double part[PNP_LM_LANES][28];
  __shared__ double J[PNP_LM_LANES][12];
  __shared__ double o[PNP_LM_LANES][28];
  __shared__ double tot[28], S[PL_SIZE], M[12], sK[4];
  __shared__ uint8_t msk[PNP_MAX_POINTS];
  __shared__ int sh[2];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = clamp_count(a.n[b], a.ncap);
  uint8_t* mask = a.mask + (size_t)b * a.mcap;
  for (int i = t; i < a.mcap; i += PNP_LM_LANES) mask[i] = 0;
  if (t == 0) {
    sK[0] = a.fx; sK[1] = a.fy; sK[2] = a.cx; sK[3] = a.cy;
    int best = 0;
    sh[0] = n >= PNP_MIN_POINTS ? pnp_select(a.scores + (size_t)b * PNP_MAX_ITERS, n, &best) : -1;
    sh[1] = best;
  }
  __syncthreads();
  const int win = sh[0];
  double* Twc = a.Twc + 16 * (size_t)b;
  double* Rt = a.Rt ? a.Rt + 12 * (size_t)b : nullptr;
  if (win < 0) {                                             // no model: count 0, identity pose, an all-zero mask
    if (t < 16) Twc[t] = (t % 5) == 0 ? 1.0 : 0.0;
    if (Rt && t < 12) Rt[t] = (t == 0 || t == 4 || t == 8) ? 1.0 : 0.0;
    if (t == 0) a.count[b] = 0;
    return;
  }
  const float* obj = a.obj + (size_t)b * a.ncap * 3;
  const float* img = a.img + (size_t)b * a.ncap * 2;
  if (t < 12) M[t] = a.models[((size_t)b * PNP_MAX_ITERS + win) * 12 + t];
  __syncthreads();
  for (int i = t; i < n; i += PNP_LM_LANES)
    msk[i] = pnp_error(M, obj[3 * i], obj[3 * i + 1], obj[3 * i + 2], img[2 * i], img[2 * i + 1], sK) <= PNP_THRESH2;
  __syncthreads();
  lm_accumulate(M, obj, img, msk, n, sK, part, J, o, tot);
  if (t == 0) pnp_lm_start(S, M, tot);
  __syncthreads();
  for (int it = 0; it < PNP_LM_ITERS; ++it) {
    if (S[PL_STOP] != 0.0) break;
    if (t == 0) pnp_lm_propose(S);
    __syncthreads();
    if (S[PL_STOP] != 0.0) break;
    lm_accumulate(S + PL_TRY, obj, img, msk, n, sK, part, J, o, tot);
    if (t == 0) pnp_lm_judge(S, tot);
    __syncthreads();
  }
  if (t == 0) {
    const double* res = pnp_finite12(S + PL_CUR) ? S + PL_CUR : M;
    pnp_twc(res, Twc);
    if (Rt)
      for (int k = 0; k < 12; ++k) Rt[k] = res[k];
    a.count[b] = sh[1];
  }
  const int* map = a.map ? a.map + (size_t)b * a.ncap : nullptr;
  for (int i = t; i < n; i += PNP_LM_LANES) mask[map ? map[i] : i] = msk[i];
}

__global__ __launch_bounds__(256) void pnp_gather_kernel(PnpGatherArgs g) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int m = clamp_count(g.ntrack[b], g.mcap);
  const int32_t* tidx = g.tidx + (size_t)b * g.mcap * 2;
  float* obj = g.obj + (size_t)b * g.ncap * 3;
  float* img = g.img + (size_t)b * g.ncap * 2;
  int* map = g.map + (size_t)b * g.ncap;
  int kept = 0;
  for (int base = 0; base < m; base += 256) {
    const int j = base + t;
    bool valid = false;
    float X = 0.f, Y = 0.f, Z = 0.f, u = 0.f, v = 0.f;
    if (j < m) {
      const int r = tidx[2 * j], c = tidx[2 * j + 1];
      if (r >= 0 && r < g.capK && c >= 0 && c < g.cap) {        // the matcher's indices are in range; this is memory safety only
        const double* p = g.xyz + ((size_t)b * g.capK + r) * 3;
        valid = !is_nan(p[0]);
        X = (float)p[0]; Y = (float)p[1]; Z = (float)p[2];
        const float* f = g.feat + ((size_t)b * g.cap + c) * 259;
        u = f[1]; v = f[2];
      }
    }
    int total;
    const int q = kept + block_compact<256>(valid, wsum, &total);
    if (valid) {
      obj[3 * q] = X; obj[3 * q + 1] = Y; obj[3 * q + 2] = Z;
      img[2 * q] = u; img[2 * q + 1] = v;
      map[q] = j;
    }
    kept += total;
  }
  if (t == 0) g.n[b] = kept;
}

__global__ __launch_bounds__(256) void pnp_stereo_kernel(StereoArgs s) {
  __shared__ int last[PNP_STEREO_CAP];
  __shared__ int wgood[4];
  __shared__ double cam[8];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nl = clamp_count(s.nl[b], s.cap), nr = clamp_count(s.nr[b], s.cap), m = clamp_count(s.nmatch[b], s.mcap);
  if (t == 0) {
    cam[0] = s.min_x_diff; cam[1] = s.max_x_diff; cam[2] = s.max_y_diff; cam[3] = s.bf;
    cam[4] = s.fx; cam[5] = s.fy; cam[6] = s.cx; cam[7] = s.cy;
  }
  for (int i = t; i < s.cap; i += 256) last[i] = -1;
  __syncthreads();
  const float* fl = s.fl + (size_t)b * s.cap * 259;
  const float* fr = s.fr + (size_t)b * s.cap * 259;
  const int32_t* idx = s.idx + (size_t)b * s.mcap * 2;
  int good = 0;
  for (int j = t; j < m; j += 256) {
    const int l = idx[2 * j], r = idx[2 * j + 1];
    if (l < 0 || l >= nl || r < 0 || r >= nr) continue;      // (the host entry rejects such lists; memory safety only)
    const float* a = fl + (size_t)l * 259;
    const float* c = fr + (size_t)r * 259;
    if (pnp_stereo_good(a[1], a[2], c[1], c[2], cam)) {
      ++good;
      atomicMax(&last[l], j);                                  // a later list entry overwrites an earlier one (frame.cc:161-172)
    }
  }
  good = block_sum<256>(good, wgood);                          // (its first barrier: every atomicMax on last[] is done)
  double* ur = s.u_right + (size_t)b * s.cap;
  double* dp = s.depth + (size_t)b * s.cap;
  double* xyz = s.xyz + (size_t)b * s.cap * 3;
  for (int i = t; i < s.cap; i += 256) {
    const int j = i < nl ? last[i] : -1;
    if (j >= 0) {
      const float* a = fl + (size_t)i * 259;
      const float* c = fr + (size_t)idx[2 * j + 1] * 259;
      double q[5];
      pnp_stereo_point(a[1], a[2], c[1], cam, q);
      ur[i] = q[0]; dp[i] = q[1]; xyz[3 * i] = q[2]; xyz[3 * i + 1] = q[3]; xyz[3 * i + 2] = q[4];
    } else {
      ur[i] = -1.0; dp[i] = -1.0; xyz[3 * i] = xyz[3 * i + 1] = xyz[3 * i + 2] = quiet_nan();
    }
  }
  if (t == 0) s.good[b] = good;
}

}  // namespace

void launch_pnp(const PnpArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(pnp_models_kernel, dim3(PNP_CHUNKS, B), dim3(64), 0, st, a);
  hipLaunchKernelGGL(pnp_refine_kernel, dim3(B), dim3(PNP_LM_LANES), 0, st, a);
}
void launch_pnp_gather(const PnpGatherArgs& g, int B, hipStream_t st) {
  hipLaunchKernelGGL(pnp_gather_kernel, dim3(B), dim3(256), 0, st, g);
}
void launch_stereo_points(const StereoArgs& s, int B, hipStream_t st) {
  hipLaunchKernelGGL(pnp_stereo_kernel, dim3(B), dim3(256), 0, st, s);
}

}  // namespace airfe
