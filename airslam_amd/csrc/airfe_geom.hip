// airfe — the geometry entries of libairfe.so (include/airfe.h): F-matrix RANSAC, PnP RANSAC, stereo back-projection, track pose, the pose-only frame
// optimisation and stereo line triangulation, each as a *_queue function on a stream (the composites of airfe_bowdb.hip / airfe_junction.hip and the keyframe / track entries of airfe_frame.hip queue the same code)
// and its host and batch entries.
#include "airfe_host.h"
#include "fransac_core.h"
#include "pnp_core.h"
#include "poseopt_core.h"

// F-matrix RANSAC (src/point_matcher.cc:95-104) over B device match lists, in place, on `st` (kernels_fransac.hip).  Its scratch grows only behind
// a synchronisation of the stream it was last used on (one stream at a time per context: the contract of every *_dev entry).
int fransac_queue(airfe_ctx* c, const float* d_f0, const float* d_f1, int B, int cap, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, double* d_F,
                  hipStream_t st) {
  Carve k;
  const size_t o_scores = k.take((size_t)B * FR_RANSAC_ITERS * 3 * 4), o_state = k.take((size_t)B * 16);
  if (k.into(c, c->fr_scratch, st)) return 1;
  FransacArgs a;
  a.f0 = d_f0; a.f1 = d_f1; a.cap = cap; a.mcap = mcap; a.idx = d_idx; a.score = d_score; a.nmatch = d_nmatch; a.F = d_F;
  a.scores = k.i(o_scores);
  a.state = k.i(o_state);
  launch_fransac(a, B, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

extern "C" {

int airfe_fundamental_ransac_batch_dev(airfe_ctx* c, const float* d_f0, const int* d_n0, const float* d_f1, const int* d_n1, int B, int cap, int32_t* d_idx,
                                       float* d_score, int mcap, int* d_nmatch, double* d_F, void* stream) try {
  AIRFE_ENTER(c);
  (void)d_n0; (void)d_n1;
  if (B < 1 || cap < 1 || mcap < 1 || !d_f0 || !d_f1 || !d_idx || !d_score || !d_nmatch) return fail(c, "fundamental_ransac_batch_dev: bad argument");
  if (mcap > FR_MAX_MATCHES) return fail(c, "fundamental_ransac_batch_dev: mcap > 1024");
  return fransac_queue(c, d_f0, d_f1, B, cap, d_idx, d_score, mcap, d_nmatch, d_F, stream_of(c, stream));
} AIRFE_CATCH(c)

int airfe_fundamental_ransac(airfe_ctx* c, const float* f0, int n0, const float* f1, int n1, int32_t* idx, float* score, int m, int* kept) try {
  AIRFE_ENTER(c);
  if (!kept || m < 0 || n0 < 0 || n1 < 0 || (m > 0 && (!idx || !score || !f0 || !f1))) return fail(c, "fundamental_ransac: bad argument");
  if (m > FR_MAX_MATCHES) return fail(c, "fundamental_ransac: more than 1024 matches");
  for (int i = 0; i < m; ++i)                                        // the reference indexes the feature matrices with these
    if (idx[2 * i] < 0 || idx[2 * i] >= n0 || idx[2 * i + 1] < 0 || idx[2 * i + 1] >= n1) return fail(c, "fundamental_ransac: match index out of range");
  *kept = m;
  if (m < 9) return 0;                                               // point_matcher.cc:95: the list as it is (the kernels' gate says the same)
  const int cap = std::max(n0, n1);
  hipStream_t st = c->stream;
  Carve k;
  const size_t fb = (size_t)cap * AIRFE_FEAT_DIM * 4;
  const size_t o_nm = k.take(4), o_f0 = k.take(fb), o_f1 = k.take(fb), o_idx = k.take((size_t)m * 8), o_sc = k.take((size_t)m * 4);
  if (k.into(c, c->fr_stage, st)) return 1;
  int* d_nm = k.i(o_nm);
  float *d_f0 = k.at<float>(o_f0), *d_f1 = k.at<float>(o_f1), *d_sc = k.at<float>(o_sc);
  int32_t* d_idx = k.at<int32_t>(o_idx);
  DrainOnError drain{c, true};
  HIPCHK(c, hipMemcpyAsync(d_nm, &m, 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_f0, f0, (size_t)n0 * AIRFE_FEAT_DIM * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_f1, f1, (size_t)n1 * AIRFE_FEAT_DIM * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_idx, idx, (size_t)m * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_sc, score, (size_t)m * 4, hipMemcpyHostToDevice, st));
  if (fransac_queue(c, d_f0, d_f1, 1, cap, d_idx, d_sc, m, d_nm, nullptr, st)) return 1;
  int nk = 0;
  HIPCHK(c, hipMemcpyAsync(&nk, d_nm, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (nk > 0) {
    HIPCHK(c, hipMemcpyAsync(idx, d_idx, (size_t)nk * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(score, d_sc, (size_t)nk * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  drain.armed = false;
  *kept = nk;
  return 0;
} AIRFE_CATCH(c)

int airfe_set_outlier_rejection(airfe_ctx* c, int on) try {
  AIRFE_ENTER(c);
  c->outlier_rejection = on != 0;
  return 0;
} AIRFE_CATCH(c)

}  // extern "C"

// PnP RANSAC (g2o_optimization.cc:1085-1134) over B device problems on `st` (kernels_pnp.hip): scores + models of the 100 samples in the context's
// scratch (grown only behind a synchronisation of the stream it was last used on, as fransac_queue's).
int pnp_queue(airfe_ctx* c, const float* d_obj, const float* d_img, const int* d_n, int B, int ncap, const double* K, double* d_Twc, double* d_Rt, uint8_t* d_mask,
              int mcap, const int* d_map, int* d_count, hipStream_t st) {
  Carve k;
  const size_t o_scores = k.take((size_t)B * PNP_MAX_ITERS * 4), o_models = k.take((size_t)B * PNP_MAX_ITERS * 12 * 8);
  if (k.into(c, c->pn_scratch, st)) return 1;
  PnpArgs a;
  a.obj = d_obj; a.img = d_img; a.n = d_n; a.ncap = ncap;
  a.fx = K[0]; a.fy = K[1]; a.cx = K[2]; a.cy = K[3];
  a.scores = k.i(o_scores);
  a.models = k.d(o_models);
  a.Twc = d_Twc; a.Rt = d_Rt; a.mask = d_mask; a.mcap = mcap; a.map = d_map; a.count = d_count;
  launch_pnp(a, B, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

extern "C" {

int airfe_pnp_ransac_batch_dev(airfe_ctx* c, const float* d_obj, const float* d_img, const int* d_n, int B, int ncap, const double* K, double* d_Twc,
                               double* d_Rt, uint8_t* d_inlier, int* d_count, void* stream) try {
  AIRFE_ENTER(c);
  if (B < 1 || ncap < 1 || !d_obj || !d_img || !d_n || !K || !d_Twc || !d_inlier || !d_count) return fail(c, "pnp_ransac_batch_dev: bad argument");
  if (ncap > PNP_MAX_POINTS) return fail(c, "pnp_ransac_batch_dev: ncap > 1024");
  return pnp_queue(c, d_obj, d_img, d_n, B, ncap, K, d_Twc, d_Rt, d_inlier, ncap, nullptr, d_count, stream_of(c, stream));
} AIRFE_CATCH(c)

int airfe_pnp_ransac(airfe_ctx* c, const double* obj, const double* img, int n, const double* K, double* Twc, double* Rt, uint8_t* inlier, int* count) try {
  AIRFE_ENTER(c);
  if (n < 0 || !K || !Twc || !count || (n > 0 && (!obj || !img || !inlier))) return fail(c, "pnp_ransac: bad argument");
  if (n > PNP_MAX_POINTS) return fail(c, "pnp_ransac: more than 1024 correspondences");
  const int ncap = std::max(n, 1);
  // one block: n | Twc [16] | Rt [12] | count | obj [ncap][3] f32 with img [ncap][2] f32 right behind it (they go up in one copy) | mask [ncap]
  hipStream_t st = c->stream;
  Carve kc;
  const size_t o_n = kc.take(4), o_Twc = kc.take(128), o_Rt = kc.take(96), o_count = kc.take(4), o_pts = kc.take((size_t)ncap * 20), o_mask = kc.take(ncap);
  if (kc.into(c, c->pn_stage, st)) return 1;
  std::vector<float> h((size_t)ncap * 5, 0.f);
  for (int i = 0; i < n; ++i) {                                      // cv::Point3f / cv::Point2f: the doubles rounded to float
    for (int k = 0; k < 3; ++k) h[3 * i + k] = (float)obj[3 * i + k];
    for (int k = 0; k < 2; ++k) h[(size_t)ncap * 3 + 2 * i + k] = (float)img[2 * i + k];
  }
  int *d_n = kc.i(o_n), *d_count = kc.i(o_count);
  double *d_Twc = kc.d(o_Twc), *d_Rt = kc.d(o_Rt);
  float *d_obj = kc.at<float>(o_pts), *d_img = d_obj + (size_t)ncap * 3;
  uint8_t* d_mask = kc.at<uint8_t>(o_mask);
  DrainOnError drain{c, true};
  HIPCHK(c, hipMemcpyAsync(d_n, &n, 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_obj, h.data(), (size_t)ncap * 20, hipMemcpyHostToDevice, st));
  if (pnp_queue(c, d_obj, d_img, d_n, 1, ncap, K, d_Twc, d_Rt, d_mask, ncap, nullptr, d_count, st)) return 1;
  double rt[12];
  HIPCHK(c, hipMemcpyAsync(Twc, d_Twc, 128, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(rt, d_Rt, 96, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(count, d_count, 4, hipMemcpyDeviceToHost, st));
  if (n > 0) HIPCHK(c, hipMemcpyAsync(inlier, d_mask, n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  drain.armed = false;
  if (Rt) memcpy(Rt, rt, 96);
  return 0;
} AIRFE_CATCH(c)

int airfe_stereo_points(airfe_ctx* c, const double* cam, const float* featL, int nL, const float* featR, int nR, const int32_t* idx, int m, double* u_right,
                        double* depth, double* xyz, int* good) try {
  if (!c) return 1;
  if (!cam || !good || nL < 0 || nR < 0 || m < 0 || (nL > 0 && (!featL || !u_right || !depth || !xyz)) || (m > 0 && (!idx || !featR)))
    return fail(c, "stereo_points: bad argument");
  for (int j = 0; j < m; ++j)                                        // Frame::AddRightFeatures indexes both feature matrices with these
    if (idx[2 * j] < 0 || idx[2 * j] >= nL || idx[2 * j + 1] < 0 || idx[2 * j + 1] >= nR) return fail(c, "stereo_points: match index out of range");
  *good = pnp_stereo_host(featL, nL, featR, idx, m, cam, u_right, depth, xyz);
  return 0;
} AIRFE_CATCH(c)

int airfe_stereo_points_batch_dev(airfe_ctx* c, const double* cam, const float* d_featL, const int* d_nL, const float* d_featR, const int* d_nR, int B,
                                  int cap, const int32_t* d_idx, const int* d_nmatch, int mcap, double* d_u_right, double* d_depth, double* d_xyz,
                                  int* d_good, void* stream) try {
  AIRFE_ENTER(c);
  if (B < 1 || cap < 1 || mcap < 1 || !cam || !d_featL || !d_nL || !d_featR || !d_nR || !d_idx || !d_nmatch || !d_u_right || !d_depth || !d_xyz || !d_good)
    return fail(c, "stereo_points_batch_dev: bad argument");
  if (cap > PNP_STEREO_CAP) return fail(c, "stereo_points_batch_dev: cap > 4096");
  StereoArgs s;
  s.fl = d_featL; s.fr = d_featR; s.nl = d_nL; s.nr = d_nR; s.cap = cap; s.idx = d_idx; s.nmatch = d_nmatch; s.mcap = mcap;
  s.min_x_diff = cam[0]; s.max_x_diff = cam[1]; s.max_y_diff = cam[2]; s.bf = cam[3]; s.fx = cam[4]; s.fy = cam[5]; s.cx = cam[6]; s.cy = cam[7];
  s.u_right = d_u_right; s.depth = d_depth; s.xyz = d_xyz; s.good = d_good;
  launch_stereo_points(s, B, stream_of(c, stream));
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(c)

// The gathered PnP problems of both track-pose entries in the context's pn_gather: obj [B][mcap][3] | img [B][mcap][2] f32 | map [B][mcap] | n [B]; g comes
// back with the arrays' addresses
static int pnp_gather_queue(airfe_ctx* c, const double* d_xyz, int capK, const float* d_feat, int cap, const int32_t* d_tidx, const int* d_ntrack, int mcap, int B,
                            PnpGatherArgs& g, hipStream_t st) {
  Carve k;
  const size_t o_obj = k.take((size_t)B * mcap * 12), o_img = k.take((size_t)B * mcap * 8), o_map = k.take((size_t)B * mcap * 4), o_n = k.take((size_t)B * 4);
  if (k.into(c, c->pn_gather, st)) return 1;
  g.xyz = d_xyz; g.capK = capK; g.feat = d_feat; g.cap = cap; g.tidx = d_tidx; g.ntrack = d_ntrack; g.mcap = mcap; g.ncap = mcap;
  g.obj = k.at<float>(o_obj); g.img = k.at<float>(o_img); g.map = k.i(o_map); g.n = k.i(o_n);
  launch_pnp_gather(g, B, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_track_pose_batch_dev(airfe_ctx* c, const double* K, const double* d_xyz, int capK, const float* d_feat, int cap, const int32_t* d_tidx,
                               const int* d_ntrack, int mcap, int B, double* d_Twc, double* d_Rt, uint8_t* d_mask, int* d_count, void* stream) try {
  AIRFE_ENTER(c);
  if (B < 1 || capK < 1 || cap < 1 || mcap < 1 || !K || !d_xyz || !d_feat || !d_tidx || !d_ntrack || !d_Twc || !d_mask || !d_count)
    return fail(c, "track_pose_batch_dev: bad argument");
  if (mcap > PNP_MAX_POINTS) return fail(c, "track_pose_batch_dev: mcap > 1024");
  hipStream_t st = stream_of(c, stream);
  PnpGatherArgs g;
  if (pnp_gather_queue(c, d_xyz, capK, d_feat, cap, d_tidx, d_ntrack, mcap, B, g, st)) return 1;
  return pnp_queue(c, g.obj, g.img, g.n, B, mcap, K, d_Twc, d_Rt, d_mask, mcap, g.map, d_count, st);
} AIRFE_CATCH(c)

}  // extern "C"

// Pose-only frame optimisation (g2o_optimization.cc:446-898, one free pose, point edges) over B device problems on `st` (kernels_poseopt.hip)
int poseopt_queue(airfe_ctx* c, const double* d_X, const double* d_obs, const int* d_n, int B, int ncap, const double* d_Twc0, const double* cam, const double* Tcb,
                  const double* thr, double* d_Twc, double* d_Rt, uint8_t* d_inlier, int mcap, const int* d_map, int* d_num, int lost, int* d_ok, hipStream_t st) {
  PoseoptArgs a;
  a.X = d_X; a.obs = d_obs; a.n = d_n; a.ncap = ncap; a.Twc0 = d_Twc0;
  for (int k = 0; k < 5; ++k) a.cam[k] = cam[k];
  for (int k = 0; k < 2; ++k) a.thr[k] = thr[k];
  if (Tcb) {
    for (int k = 0; k < 12; ++k) a.Tcb[k] = Tcb[k];
    a.has_tcb = 1;
  }
  a.Twc = d_Twc; a.Rt = d_Rt; a.inlier = d_inlier; a.mcap = mcap; a.map = d_map; a.num = d_num; a.lost = lost; a.ok = d_ok;
  launch_poseopt(a, B, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

extern "C" {

int airfe_frame_optimize_batch_dev(airfe_ctx* c, const double* d_X, const double* d_obs, const int* d_n, int B, int ncap, const double* d_Twc0,
                                   const double* cam, const double* Tcb, const double* thr, double* d_Twc, double* d_Rt, uint8_t* d_inlier, int* d_num,
                                   void* stream) try {
  AIRFE_ENTER(c);
  if (B < 1 || ncap < 1 || !d_X || !d_obs || !d_n || !d_Twc0 || !cam || !thr || !d_Twc || !d_inlier || !d_num)
    return fail(c, "frame_optimize_batch_dev: bad argument");
  if (ncap > PO_MAX_POINTS) return fail(c, "frame_optimize_batch_dev: ncap > 1024");
  return poseopt_queue(c, d_X, d_obs, d_n, B, ncap, d_Twc0, cam, Tcb, thr, d_Twc, d_Rt, d_inlier, ncap, nullptr, d_num, -1, nullptr,
                       stream_of(c, stream));
} AIRFE_CATCH(c)

int airfe_frame_optimize(airfe_ctx* c, const double* X, const double* obs, int n, const double* cam, const double* Tcb, const double* thr,
                         const double* Twc0, double* Twc, double* Rt, uint8_t* inlier, int* num_inliers) try {
  AIRFE_ENTER(c);
  if (n < 0 || !cam || !thr || !Twc0 || !Twc || !num_inliers || (n > 0 && (!X || !obs || !inlier))) return fail(c, "frame_optimize: bad argument");
  if (n > PO_MAX_POINTS) return fail(c, "frame_optimize: more than 1024 constraints");
  const int ncap = std::max(n, 1);
  // one block: n | Twc0 [16] | Twc [16] | Rt [12] | num | X [ncap][3] | obs [ncap][3] | inlier [ncap]
  hipStream_t st = c->stream;
  Carve k;
  const size_t o_n = k.take(4), o_Twc0 = k.take(128), o_Twc = k.take(128), o_Rt = k.take(96), o_num = k.take(4), o_X = k.take((size_t)ncap * 24),
               o_obs = k.take((size_t)ncap * 24), o_mask = k.take(ncap);
  if (k.into(c, c->po_stage, st)) return 1;
  int *d_n = k.i(o_n), *d_num = k.i(o_num);
  double *d_Twc0 = k.d(o_Twc0), *d_Twc = k.d(o_Twc), *d_Rt = k.d(o_Rt), *d_X = k.d(o_X), *d_obs = k.d(o_obs);
  uint8_t* d_mask = k.at<uint8_t>(o_mask);
  DrainOnError drain{c, true};
  HIPCHK(c, hipMemcpyAsync(d_n, &n, 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_Twc0, Twc0, 128, hipMemcpyHostToDevice, st));
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(d_X, X, (size_t)n * 24, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_obs, obs, (size_t)n * 24, hipMemcpyHostToDevice, st));
  }
  if (poseopt_queue(c, d_X, d_obs, d_n, 1, ncap, d_Twc0, cam, Tcb, thr, d_Twc, d_Rt, d_mask, ncap, nullptr, d_num, -1, nullptr, st)) return 1;
  double rt[12];
  HIPCHK(c, hipMemcpyAsync(Twc, d_Twc, 128, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(rt, d_Rt, 96, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(num_inliers, d_num, 4, hipMemcpyDeviceToHost, st));
  if (n > 0) HIPCHK(c, hipMemcpyAsync(inlier, d_mask, n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  drain.armed = false;
  if (Rt) memcpy(Rt, rt, 96);
  return 0;
} AIRFE_CATCH(c)

int airfe_track_pose_opt_batch_dev(airfe_ctx* c, const double* cam, const double* thr, int lost_num_match, const double* d_xyz, int capK,
                                   const float* d_feat, int cap, const int32_t* d_tidx, const int* d_ntrack, int mcap, int B, const double* d_u_right,
                                   const double* d_Twc_last, double* d_Twc, double* d_Rt, uint8_t* d_mask, int* d_num, int* d_ok, int* d_pnp_count,
                                   void* stream) try {
  AIRFE_ENTER(c);
  if (B < 1 || capK < 1 || cap < 1 || mcap < 1 || lost_num_match < 0 || !cam || !thr || !d_xyz || !d_feat || !d_tidx || !d_ntrack || !d_Twc || !d_mask ||
      !d_num || !d_ok)
    return fail(c, "track_pose_opt_batch_dev: bad argument");
  if (mcap > PNP_MAX_POINTS) return fail(c, "track_pose_opt_batch_dev: mcap > 1024");
  hipStream_t st = stream_of(c, stream);
  // this entry's block: X [B][mcap][3] | obs [B][mcap][3] | Twc_pnp [B][16] | Twc0 [B][16] f64 | pnp count [B] | pnp mask [B][mcap]
  Carve k;
  const size_t o_X = k.take((size_t)B * mcap * 24), o_obs = k.take((size_t)B * mcap * 24), o_pnp = k.take((size_t)B * 128), o_seed = k.take((size_t)B * 128),
               o_cnt = k.take((size_t)B * 4), o_msk = k.take((size_t)B * mcap);
  if (k.into(c, c->po_gather, st)) return 1;
  PnpGatherArgs g;
  if (pnp_gather_queue(c, d_xyz, capK, d_feat, cap, d_tidx, d_ntrack, mcap, B, g, st)) return 1;
  double* d_pnp = k.d(o_pnp);
  int* d_cnt = d_pnp_count ? d_pnp_count : k.i(o_cnt);
  if (pnp_queue(c, g.obj, g.img, g.n, B, mcap, cam, d_pnp, nullptr, k.at<uint8_t>(o_msk), mcap, g.map, d_cnt, st)) return 1;
  PoseoptGatherArgs q;
  q.xyz = d_xyz; q.capK = capK; q.feat = d_feat; q.cap = cap; q.tidx = d_tidx; q.mcap = mcap; q.map = g.map; q.n = g.n; q.ncap = mcap;
  q.u_right = d_u_right; q.Twc_pnp = d_pnp; q.Twc_last = d_Twc_last; q.pnp_count = d_cnt; q.lost = lost_num_match;
  q.X = k.d(o_X); q.obs = k.d(o_obs); q.Twc0 = k.d(o_seed);
  launch_poseopt_gather(q, B, st);
  HIPCHK(c, hipGetLastError());
  return poseopt_queue(c, q.X, q.obs, g.n, B, mcap, q.Twc0, cam, nullptr, thr, d_Twc, d_Rt, d_mask, mcap, g.map, d_num, lost_num_match, d_ok, st);
} AIRFE_CATCH(c)

}  // extern "C"

// Stereo line triangulation (frame.cc:185-191, line_processor.cc:196-245, :312-326) over B device frames on `st` (kernels_stereoline.hip): the counts are
// zeroed on the stream, then one launch.  No scratch, nothing allocated.
int stereo_lines_queue(airfe_ctx* c, const double* cam, const double* d_left, const int* d_nl, const double* d_right, const int* d_nr, int capL,
                       const int32_t* d_matches, const double* d_Twc, int B, double* d_sel, uint8_t* d_valid, int32_t* d_status, double* d_endpoints,
                       double* d_plucker, int32_t* d_count, hipStream_t st) {
  StereoLineArgs a;
  a.left = d_left; a.right = d_right; a.nl = d_nl; a.nr = d_nr; a.capL = capL; a.matches = d_matches; a.Twc = d_Twc;
  for (int k = 0; k < 8; ++k) a.cam[k] = cam[k];
  a.sel = d_sel; a.valid = d_valid; a.status = d_status; a.endpoints = d_endpoints; a.plucker = d_plucker; a.count = d_count;
  ProfScope ps(c, ST_LINE_ASSOC, st, 0, (double)B * (double)capL * 176);
  HIPCHK(c, hipMemsetAsync(d_count, 0, (size_t)B * 12, st));
  launch_stereo_lines(a, B, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

extern "C" {

int airfe_stereo_lines(airfe_ctx* c, const double* cam, const double* lines_left, int nL, const double* lines_right, int nR, const int32_t* line_matches,
                       const double* Twc, double* lines_right_sel, uint8_t* right_valid, int32_t* status, double* endpoints, double* plucker,
                       int32_t* count) try {
  if (!c) return 1;
  if (!cam || !count || nL < 0 || nR < 0 || (nR > 0 && !lines_right) ||
      (nL > 0 && (!lines_left || !line_matches || !lines_right_sel || !right_valid || !status || !endpoints || !plucker)))
    return fail(c, "stereo_lines: bad argument");
  stereo_lines_host(cam, lines_left, nL, lines_right, nR, line_matches, Twc, lines_right_sel, right_valid, status, endpoints, plucker, count);
  return 0;
} AIRFE_CATCH(c)

int airfe_stereo_lines_batch_dev(airfe_ctx* c, const double* cam, const double* d_lines_left, const int* d_nlines_left, const double* d_lines_right,
                                 const int* d_nlines_right, int capL, const int32_t* d_line_matches, const double* d_Twc, int B, double* d_lines_right_sel,
                                 uint8_t* d_right_valid, int32_t* d_status, double* d_endpoints, double* d_plucker, int32_t* d_count, void* stream) try {
  AIRFE_ENTER(c);
  if (B < 1 || B > 65535 || capL < 1 || !cam || !d_lines_left || !d_nlines_left || !d_lines_right || !d_nlines_right || !d_line_matches)
    return fail(c, "stereo_lines_batch_dev: bad argument");
  if (!d_lines_right_sel || !d_right_valid || !d_status || !d_endpoints || !d_plucker || !d_count) return fail(c, "stereo_lines_batch_dev: null output");
  return stereo_lines_queue(c, cam, d_lines_left, d_nlines_left, d_lines_right, d_nlines_right, capL, d_line_matches, d_Twc, B, d_lines_right_sel,
                            d_right_valid, d_status, d_endpoints, d_plucker, d_count, stream_of(c, stream));
} AIRFE_CATCH(c)

int airfe_stereo_line_landmarks_batch_dev(airfe_ctx* c, const double* cam, const double* d_lines_left, const int* d_nlines_left, const double* d_lines_right,
                                          const int* d_nlines_right, int capL, const float* d_featL, const int* d_nL, const float* d_featR, const int* d_nR,
                                          int cap, const int32_t* d_idx, const int* d_nmatch, int mcap, const double* d_Twc, int B, int32_t* d_row_ptrL,
                                          int32_t* d_pt_idxL, double* d_pt_distL, int* d_totalL, int32_t* d_row_ptrR, int32_t* d_pt_idxR, double* d_pt_distR,
                                          int* d_totalR, int capE, int32_t* d_line_matches, double* d_lines_right_sel, uint8_t* d_right_valid,
                                          int32_t* d_status, double* d_endpoints, double* d_plucker, int32_t* d_count, void* stream) try {
  AIRFE_ENTER(c);
  if (B < 1 || B > 65535 || capL < 1 || cap < 1 || mcap < 1 || capE < 1 || !cam || !d_lines_left || !d_nlines_left || !d_lines_right || !d_nlines_right ||
      !d_featL || !d_nL || !d_featR || !d_nR || !d_idx || !d_nmatch)
    return fail(c, "stereo_line_landmarks_batch_dev: bad argument");
  if (!d_row_ptrL || !d_pt_idxL || !d_pt_distL || !d_row_ptrR || !d_pt_idxR || !d_pt_distR || !d_line_matches || !d_lines_right_sel || !d_right_valid ||
      !d_status || !d_endpoints || !d_plucker || !d_count)
    return fail(c, "stereo_line_landmarks_batch_dev: null output");
  void* st = stream ? stream : (void*)c->stream;
  // frame.cc:125, :177, :184 through the entries a caller would chain by hand, unchanged (association and match have no *_queue function: their public
  // entries are called as they are, each with its own argument check, device check and catch, and its own scratch block in the context, which grows
  // behind a stream synchronisation on the first call or a larger shape); then the loop of :185-191 and Map::InsertKeyframe's (map.cc:81-95)
  if (airfe_assign_points_to_lines_batch_dev(c, d_lines_left, d_nlines_left, capL, d_featL, d_nL, cap, B, d_row_ptrL, d_pt_idxL, d_pt_distL, capE, d_totalL, st))
    return 1;
  if (airfe_assign_points_to_lines_batch_dev(c, d_lines_right, d_nlines_right, capL, d_featR, d_nR, cap, B, d_row_ptrR, d_pt_idxR, d_pt_distR, capE, d_totalR,
                                             st))
    return 1;
  if (airfe_match_lines_batch_dev(c, d_row_ptrL, d_pt_idxL, d_nlines_left, d_nL, d_row_ptrR, d_pt_idxR, d_nlines_right, d_nR, capL, capE, d_idx, d_nmatch, mcap,
                                  B, cam, d_featL, d_featR, cap, d_line_matches, st))
    return 1;
  return stereo_lines_queue(c, cam, d_lines_left, d_nlines_left, d_lines_right, d_nlines_right, capL, d_line_matches, d_Twc, B, d_lines_right_sel, d_right_valid,
                            d_status, d_endpoints, d_plucker, d_count, (hipStream_t)st);
} AIRFE_CATCH(c)

}  // extern "C"
