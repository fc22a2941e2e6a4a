/* airfe — C ABI of the MI355X-native per-frame front end (feature detect + match) for AirSLAM.
 *
 * This header is the drop-in boundary: every entry point names the reference interface it
 * replaces (paths under the AirSLAM checkout).  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - return value: 0 = ok, non-zero = failure (airfe_last_error() gives the text); never throws: every entry point catches C++ exceptions
 *     (allocation failures of its host-side bookkeeping included) at the boundary and reports them as a failure.
 *   - one ctx = one HIP stream = one calling thread (the reference wrappers are not re-entrant either:
 *     include/plnet.h:38-63, include/light_glue.h:39-47).
 *   - feature rows are 259 contiguous floats [score, x, y, d0..d255]: byte-identical to one COLUMN of the
 *     reference's column-major Eigen::Matrix<float,259,Dynamic> (include/feature_detector.h:8-31), so the
 *     C++ shim does features.resize(259,n) + one memcpy.
 *   - activation range: with 2-byte detector storage (cfg.precision 0 / 1) an activation above 65504 (fp16) overflows.  Weight packs made by tools/onnx_to_pack.py
 *     are rescaled between layers by exact powers of two (airslam_amd.weights.fold_activation_scales) so that calibration maxima sit at <= 2048; if a frame still
 *     drives the score logits or a sampled descriptor to inf / NaN, the host entries FAIL for that call (airfe_last_error says so) and the asynchronous *_dev
 *     entries report it through airfe_sync / airfe_superglue_status — keypoints of a poisoned score map are never handed out.  cfg.precision = 2 has fp32 range.
 *   - *_dev entry points take DEVICE pointers and an optional hipStream_t (NULL = the ctx stream); they are
 *     asynchronous.  They have no reference counterpart (the reference is batch-1, host buffers only).
 */
#ifndef AIRFE_H_
#define AIRFE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIRFE_FEAT_DIM 259
#define AIRFE_INTERNAL_SIZE 512 /* reference resizes every image to 512x512: src/plnet.cpp:17-18,258 */

typedef struct airfe_ctx airfe_ctx;

/* Every field: -1 = the library's default / automatic choice.  None of these changes a result beyond what the tests state (most forms are bit-identical). */
typedef struct airfe_tuning {
  int fuse_lg_block;     /* LightGlue / SuperGlue out-projection + FFN + residual as one kernel: 0 / 1 force, -1 by token count */
  int gemm_small_max_m;  /* rows up to which the no-LDS GEMM is used */
  int gemm8_min_m;       /* rows from which the 8-wave tiled GEMM is used */
  int gemmr_min_m;       /* rows from which the streaming (DMA ring) q|k|v projection is used */
  int gemmr_wgs;         /* its persistent workgroups (tests lower it so that a small batch wraps the ring) */
  int qkv_pair;          /* q|k and v of a layer in one streaming launch (1) or two (0) */
  int block_min_m;       /* tokens from which the fused block is used when fuse_lg_block = -1 */
  int lgb_tokens;        /* tokens per workgroup of the fused block: 32 / 64 / 112 / 128 */
  int sg_kenc_gemm;      /* SuperGlue keypoint encoder's large layers as GEMMs (1) or scalar loops (0) */
  int fold_qkv;          /* the next attention layer's projections inside the fused block (1) or as launches of their own (0) */
  int overlap_lines;     /* PLNet line path on a second stream beside the matcher (1) or behind it (0) */
  int kf_graph;          /* airfe_stereo_keyframe replays a captured hipGraph (1); default 0 (measured: <= 1 %) */
  int kf_spec_rows;      /* line / junction rows airfe_stereo_keyframe copies back before it knows the counts */
  int fuse_dec;          /* PLNet stage-0: 17-channel head + decode in one pass (1) or two (0) */
  int assign_fused;      /* LightGlue assignment: log-sum-exp / arg-max partials taken in the similarity tiles (1; no similarity matrix in HBM)
                            or the round-2 form: similarity matrix + four passes over it (0, the default: the A/B is in profiles/r05_assign_ab.txt) */
  int fold_out_proj;     /* LightGlue / SuperGlue: the attention out-projection (out_proj / to_out / merge) multiplied into the message half of ffn.0 / mlp.0 when
                            the weights are packed — two linear maps with nothing between them are one: W1m (Wo a + bo) = (W1m Wo) a + W1m bo — so a block runs
                            ffn.0 on cat(x, attention output) and the 256x256 GEMM, its barrier and its message tile are gone (1, the default for fp16 / bf16);
                            0: the out-projection as a GEMM of its own (the round 1-4 form; profiles/r05_fold_out_ab.txt) */
  int desc_gather_stream;/* the descriptor head over the sampled cells of a large batch (>= gemmr_min_m rows) in the streaming kernel with gathered rows (1, default)
                            or the tiled 8-wave kernel (0); the same bits (tests/test_gpu_detector.py).  Round 6: also the LOI head at the junctions' tap rows
                            (K = N = 128) and the dense descriptor head of the junction images */
  int copy_wgs;          /* airfe_copy_rows_dev: workgroups of the copy kernel (default 64: PCIe-bound copies into pinned memory need stores in flight, not CUs) */
  int reserved[5];       /* must be -1 */
} airfe_tuning;

/* Mirrors the knobs of PLNetConfig / SuperPointConfig / PointMatcherConfig (include/read_configs.h:9-103). */
typedef struct airfe_cfg {
  int device;                  /* HIP device ordinal */
  int precision;               /* detector storage type: 2 = fp32 storage AND arithmetic (correctness mode, f32-input MFMA; BASELINE configs[1]),
                                  1 = fp16 (default; the reference's engines are built with kFP16,
                                  super_point.cpp:97, plnet.cpp:216 — and the only 2-byte type that meets the 1e-3 descriptor-cosine
                                  tolerance once descriptors are decorrelated: bf16 measures 2e-2), 0 = bf16; accumulation is always fp32 */
  int max_batch;               /* images per detect batch / 2x pairs per match batch the arena is sized for */
  int enc_chunk;               /* images per pass through the full-resolution conv layers (cache blocking) */
  int max_keypoints;           /* plnet.max_keypoints        (<= 1024, light_glue.cpp:52) */
  float keypoint_threshold;    /* plnet.keypoint_threshold */
  int remove_borders;          /* plnet.remove_borders */
  int nms_radius;              /* SuperPoint simple_nms radius inside the model graph (4 upstream; 0 = off) */
  float line_threshold;        /* plnet.line_threshold */
  float line_length_threshold; /* plnet.line_length_threshold */
  int matcher;                 /* point_matcher.matcher: 0 = LightGlue, 1 = SuperGlue */
  int image_width;             /* point_matcher.image_width / image_height (NormalizeKeypoints) */
  int image_height;
  int sinkhorn_iters;          /* SuperGlue: iterations baked into the exported graph (100 upstream) */
  const char* superpoint_pack; /* weight packs (airslam_amd/weights.py format); NULL = that model is unavailable */
  const char* plnet_s1_pack;
  const char* lightglue_pack;
  const char* superglue_pack;
  int matcher_precision;       /* storage type of the LightGlue / SuperGlue tokens and weights: 1 = fp16 (default: the reference builds
                                  both matcher engines with BuilderFlag::kFP16, light_glue.cpp:115, super_glue.cpp:132; measured 8x
                                  closer to the fp32 oracle than bf16), 0 = bf16, 2 = fp32 (correctness mode, both matchers: f32-input MFMA GEMMs, exact soft-max), -1 = same as `precision` */
  int line_precision;          /* how the PLNet stage-1 LOI head's matrix products (src/plnet.cpp:468-514) are computed on the device path:
                                  3 = fp32 operands as PAIRS of fp16 values on the 2-byte MFMA (hi.hi + hi.lo + lo.hi, fp32 accumulation): the lines of the
                                      fp32 chain (scores within 2e-6, no candidate across the 0.75 threshold), on the pipe the reference runs this engine on
                                      (BuilderFlag::kFP16, src/plnet.cpp:216) without its rounding.  Range: the operands (LOI / thin / aux samples, hidden
                                      activations) are clamped to +-65504 before the split — the real head's stay below 64; a value beyond fp16's range enters
                                      as +-65504 instead of turning a line's score into NaN;
                                  2 = fp32 operands on the f32-input MFMA (157 TFLOP/s): the same lines, 1.8x the stage's time;
                                  1 = plain fp16 operands, REFUSED: emulated with the real weights it moves 0.5-0.9 % of the kept lines across the 0.75
                                      threshold (profiles/r05_s1_fp16_emulation.txt);
                                  0 = default: 3, and 2 in fp32 mode (precision = 2) */
  int check_launches;          /* 1 = hipGetLastError() behind every stage's launches: a failed launch is reported by the call that made it, with
                                  the stage's name (tests run with it); 0 = once per pipeline (default) */
  const airfe_tuning* tuning;       /* kernel-selection overrides (NULL = the library's own choices): A/B measurements and tests that must reach every
                                  kernel form.  Read once by airfe_create; the library never reads the environment. */
} airfe_cfg;

void airfe_default_cfg(airfe_cfg* cfg);
void airfe_default_tuning(airfe_tuning* t);      /* every field -1 */

/* ≙ the build() calls made by FeatureDetector / PointMatcher constructors
 *   (src/feature_detector.cc:7-34, src/point_matcher.cc:6-37): loads + packs weights, allocates the
 *   persistent device arena (replaces the per-infer cudaMalloc of 3rdparty/tensorrtbuffer, buffers.h:253-271). */
int airfe_create(const airfe_cfg* cfg, airfe_ctx** out);
void airfe_destroy(airfe_ctx* ctx);
const char* airfe_last_error(const airfe_ctx* ctx); /* ctx may be NULL (creation errors) */

/* ≙ SuperPoint::infer (src/super_point.cpp:103-144).  gray: h x w uint8, `stride` bytes per row
 *   (cv::Mat::step).  feat: caller buffer [cap][259]; *n receives the keypoint count (<= max_keypoints).
 *   x,y are in ORIGINAL image pixels.  Fails (non-zero) on an empty image, like the reference returns false. */
int airfe_detect_points(airfe_ctx* ctx, const uint8_t* gray, int h, int w, int stride, float* feat, int cap, int* n);

/* ≙ PLNet::infer (src/plnet.cpp:221-244).  Point branch as above.  Line branch: stage0 == NULL (what the shim passes) runs
 *   the stage-0 line head ON THE DEVICE when the detector pack carries it (tensors line.conv1.*, line.head.*: a HAWPv3-style
 *   head producing the Appendix A.1 tensors juncs_pred, lines_pred, iskeep, idx_junc_to_end_min/max, loi_features[_thin|_aux] —
 *   plnet_s0.onnx itself is absent from the reference checkout, so its weights here are synthetic); a non-NULL stage0 supplies
 *   those tensors from the HOST instead (known-answer tests of everything downstream).  Downstream of them wireframe_matcher
 *   :272-307, the stage-1 LOI head :468-514, the line/junction filter :519-558, junction_detector :425-448 and the rescale
 *   :569-582 run on the device.  lines: [capL][4] doubles (x1,y1,x2,y2) original pixels (std::vector<Eigen::Vector4d> layout);
 *   junc: [capJ][259].  No line branch in the pack and stage0 == NULL -> points only (counts 0).  The reference has no limit on lines
 *   or junctions: results that do not fit capL / capJ (45056 lines, 2048 junctions always do) are an ERROR, never a shorter list. */
typedef struct airfe_plnet_stage0 {
  const float* juncs_pred;          /* [300][2]        */
  const float* lines_pred;          /* [3*128*128][4]  */
  const float* iskeep;              /* [3*128*128]     */
  const float* idx_junc_to_end_min; /* [3*128*128]     */
  const float* idx_junc_to_end_max; /* [3*128*128]     */
  const float* loi_features;        /* [128][128][128] CHW */
  const float* loi_features_thin;   /* [4][128][128]   */
  const float* loi_features_aux;    /* [4][128][128]   */
} airfe_plnet_stage0;
int airfe_has_line_branch(const airfe_ctx* ctx); /* 1 when the detector pack carried line.* tensors AND stage 1 is loaded: infer() yields lines */
int airfe_detect_plnet(airfe_ctx* ctx, const uint8_t* gray, int h, int w, int stride, const airfe_plnet_stage0* stage0,
                       float* feat, int cap, int* n, double* lines, int capL, int* nlines, float* junc, int capJ,
                       int* njunc, int want_junctions);
/* ONE stereo keyframe through host buffers — the batch-1 entry for what src/map_builder.cc:85-86 does in two facade calls:
 *   _feature_detector->Detect(left, right, left_features, right_features, left_lines, right_lines, junctions)   (feature_detector.cc:97-108:
 *   PLNet::infer on the left image with junctions, on the right one without) and _point_matcher->MatchingPoints(left_features, right_features,
 *   stereo_matches, false) (point_matcher.cc:50-107 with LightGlue).
 * Both images go up in one copy, the detector runs over them as one batch of two, the line path runs beside LightGlue, the results come back in
 * two copies.  Per image / per pair the outputs are the bits airfe_detect_plnet x2 + airfe_match_lightglue (on NormalizeKeypoints'ed rows) return:
 *   featL / featR [cap >= max_keypoints][259] rows {score, x, y, desc[256]} + *nL / *nR;  linesL / linesR [capL][4] doubles + counts;
 *   juncL [capJ][259] + *njuncL (NULL: no junction detection);  match_idx [mcap >= max_keypoints][2] (left, right), match_score (the reference's
 *   DMatch::distance is 1 - score), *nmatch — match_idx == NULL: detection only (the 7-argument Detect overload alone).
 * Needs a detector arena of two images (cfg.max_batch >= 2, or the detector and LightGlue packs both loaded) and fp16 / bf16 arithmetic. */
int airfe_stereo_keyframe(airfe_ctx* ctx, const uint8_t* left, const uint8_t* right, int h, int w, int stride, float* featL, float* featR, int cap,
                          int* nL, int* nR, double* linesL, double* linesR, int capL, int* nlinesL, int* nlinesR, float* juncL, int capJ,
                          int* njuncL, int32_t* match_idx, float* match_score, int mcap, int* nmatch);
/* airfe_stereo_keyframe + the temporal match of the same frame: src/map_builder.cc:85-86 AND :96 — MatchingPoints(features_last_keyframe, left_features,
 * matches, true) — which every keyframe candidate runs as well.  The two LightGlue calls are independent, so they ride in ONE forward as a batch of two pairs
 * (at this size a forward costs the same for one pair as for two).  ref_feat [n_ref][259] = the last keyframe's features (NULL: the ones already on the device,
 * shared with airfe_track_frame); track_idx [mcap][2] = (reference index, left index), track_score, *ntrack.  Everything else as airfe_stereo_keyframe; per
 * pair the bits of two separate airfe_match_lightglue calls.  Needs cfg.max_batch >= 2.  airfe_set_outlier_rejection(ctx, 1): the track_* list (:96, `true`)
 * passes the F-matrix RANSAC on the device; the stereo list (:86, `false`) never does. */
int airfe_stereo_keyframe_tracked(airfe_ctx* ctx, const uint8_t* left, const uint8_t* right, int h, int w, int stride, float* featL, float* featR, int cap,
                                  int* nL, int* nR, double* linesL, double* linesR, int capL, int* nlinesL, int* nlinesR, float* juncL, int capJ,
                                  int* njuncL, int32_t* match_idx, float* match_score, int mcap, int* nmatch, const float* ref_feat, int n_ref,
                                  int32_t* track_idx, float* track_score, int* ntrack);
/* ONE tracked (non-keyframe) frame through host buffers — src/map_builder.cc:94-101: Detect(image_left_rect, left_features) followed by
 * MatchingPoints(features_last_keyframe, left_features, matches, true) (the F-matrix RANSAC behind the matcher, point_matcher.cc:95-104, runs on the
 * device before the list is copied back when airfe_set_outlier_rejection(ctx, 1) asks for it; default: the matcher's list).  ref_feat [n_ref][259] = the last keyframe's features: uploaded when given, KEPT on the device when NULL (pass them once per keyframe);
 * feat / *n = the new frame's features; match_idx [mcap][2] = (reference index, new index), match_score, *nmatch.  Same bits as airfe_detect_points +
 * airfe_match_lightglue on NormalizeKeypoints'ed rows.  Needs the detector and LightGlue packs in one context, fp16 / bf16. */
int airfe_track_frame(airfe_ctx* ctx, const uint8_t* gray, int h, int w, int stride, const float* ref_feat, int n_ref, float* feat, int cap, int* n,
                      int32_t* match_idx, float* match_score, int mcap, int* nmatch);

/* PROMOTION of the frame of the last airfe_track_frame — src/map_builder.cc:104-108: AddKeyframeCheck wants the normal frame as a keyframe, so the
 * feature thread runs Detect(image_right_rect, right_features) + MatchingPoints(left_features, right_features, stereo_matches, false) on it — as one queue:
 * the left features are the rows airfe_track_frame left on the device.  featR / *nR = the right image's features, match_idx [mcap][2] = (left, right).
 * Same bits as airfe_detect_points + airfe_match_lightglue on NormalizeKeypoints'ed rows.  Fails when no airfe_track_frame preceded it in this context. */
int airfe_promote_frame(airfe_ctx* ctx, const uint8_t* right, int h, int w, int stride, float* featR, int cap, int* nR, int32_t* match_idx,
                        float* match_score, int mcap, int* nmatch);
/* ≙ `_last_keyframe_feature = frame` (src/map_builder.cc:139-141) for a promoted frame: the rows of the last airfe_track_frame become the reference of the
 * following airfe_track_frame / airfe_stereo_keyframe_tracked calls (ref_feat == NULL) by a device-side copy — nothing crosses PCIe. */
int airfe_adopt_reference(airfe_ctx* ctx);

/* ≙ SuperPointLightGlue::infer (src/light_glue.cpp:120-170).  f0/f1: [n][258] rows = (x,y already normalised by
 *   PointMatcher::NormalizeKeypoints, d0..d255) — the contiguous temporary Eigen makes for bottomRows(258)
 *   at src/point_matcher.cc:67.  idx: [cap][2] (row-major, ascending in idx0), score = exp(log score). */
int airfe_match_lightglue(airfe_ctx* ctx, const float* f0, int n0, const float* f1, int n1, int32_t* idx, float* score,
                          int cap, int* nmatch);

/* ≙ SuperGlue::infer (src/super_glue.cpp:136-197).  f0/f1: [n][259] rows with normalised x,y.
 *   idx0 [n0], idx1 [n1] (-1 = unmatched), ms0 [n0], ms1 [n1] doubles (decode, src/super_glue.cpp:339-367). */
int airfe_match_superglue(airfe_ctx* ctx, const float* f0, int n0, const float* f1, int n1, int32_t* idx0, int32_t* idx1,
                          double* ms0, double* ms1);

/* ---- F-matrix RANSAC: the outlier rejection of MatchingPoints(..., outlier_rejection = true) (src/point_matcher.cc:95-104) ---------------
 * The reference calls cv::findFundamentalMat(points0, points1, cv::FM_RANSAC, 20, 0.99, inliers) when more than 8 matches are left and keeps the inliers
 * in order (matches[j++] = matches[i]).  The contract below restates the PUBLIC behaviour of OpenCV's legacy (non-USAC) FM_RANSAC path; OpenCV is not part
 * of this project's build or tests, so nothing here is checked against OpenCV and nothing claims bit-equality with it.  Its numerics are ours, on every
 * side: the HIP kernels (airslam_amd/csrc/kernels_fransac.hip), the C++ stand-in of cv::findFundamentalMat the tests run the reference's own
 * MatchingPoints against (shim/stubs/mini_support.cpp; both share airslam_amd/csrc/fransac_core.h) and the numpy restatement (tests/fransac_ref.py).
 *   input    the matched keypoints in ORIGINAL pixels, converted as the reference converts them: cv::Point is Point_<int> built from the floats, so x, y
 *            are truncated toward zero, then used as doubles.  LightGlue: the pairs in list order; SuperGlue: the mutual pairs in i order (:65-92).
 *   gate     fewer than 9 matches: the list comes back unchanged, bit for bit.
 *   samples  sample s (0, 1, ...) draws attempt a = 0, 1, ... < 64: slot k (0..6) is match floor(hi32(h) * m / 2^32) with
 *            h = splitmix64(0x2545F4914F6CDD1D ^ (s << 32 | a << 8 | k)) (splitmix64: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *            z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31).  An attempt is rejected when two slots repeat an index or any 3 of its points are
 *            collinear in either image (OpenCV's test: |dx2 dy1 - dy2 dx1| <= FLT_EPSILON (|dx1| + |dy1| + |dx2| + |dy2|)); a sample whose 64 attempts are
 *            all rejected yields no model.  The draws depend on (s, a, k, m) only: not on a pair's position in a batch or the batch size.
 *   solver   the 7-point algorithm in fp64: rows [x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1]; Gaussian elimination with partial pivoting (first
 *            largest |pivot|) over columns 0..6 (a pivot <= 1e-12 max|A| = no model), null vectors F1 = (.., 1, 0), F2 = (.., 0, 1) by back substitution;
 *            det(a F1 + (1 - a) F2) = 0 as a cubic solved in closed form (trigonometric for three real roots, Cardano for one; quadratic / linear when
 *            the leading coefficients are exactly 0), 1 or 3 models per sample in root order; F scaled so that F(2,2) = 1 where |F(2,2)| > DBL_EPSILON;
 *            models with a non-finite entry are dropped.  F is row-major with x1^T F x0 = 0.
 *   error    per match, in double: d = x1^T F x0, (a, b, .) = F x0, (a', b', .) = F^T x1, err = max(d^2 / (a'^2 + b'^2), d^2 / (a^2 + b^2)) (NaN = +inf),
 *            rounded to float.
 *   RANSAC   (15 and more matches) inlier: err <= 400.0f (20 px).  Sequentially, in sample order and root order: a model replaces the best only with
 *            STRICTLY more inliers than max(best, 6) (the first one wins ties); each replacement sets niters = RANSACUpdateNumIters(0.99, outliers / m,
 *            7, 1000); the search stops at the first sample index >= niters (at most 1000 samples).  The device scores samples in parallel; a scan over
 *            the scores in sample order selects exactly the model this sequential rule selects.
 *   LMedS    (9 to 14 matches: OpenCV's FM_RANSAC runs LMedS there) the same solver over samples 0..299 (round(log(0.01) / log(1 - 0.55^7))); the model
 *            with the smallest median error (the element of rank m / 2, float) wins, first on ties; inliers: err <= (float)sigma^2 with
 *            sigma = max(2.5 * 1.4826 * (1 + 5 / (m - 7)) * sqrt(median), 0.001); fewer than 7 inliers = no model.
 *   no model (every sample degenerate, no model above 6 inliers, LMedS below 7): nothing is kept, the count is 0.
 *   output   the kept matches in their original order, each index pair with its own score (DMatch::distance = 1 - score survives); F (optional) = the
 *            selected model, 9 doubles, zeros when there is none or the gate returned the list as it was.
 * Per pair the batch and the one-call entries give the same bytes. */
/* ≙ point_matcher.cc:95-104 on ONE pair through host buffers: f0 [n0][259], f1 [n1][259] rows (original pixels), the list idx [m][2] (index into f0, into f1)
 * + score [m], filtered in place; *kept = the new length.  m <= 1024. */
int airfe_fundamental_ransac(airfe_ctx* ctx, const float* f0, int n0, const float* f1, int n1, int32_t* idx, float* score, int m, int* kept);
/* the same over B device-resident pairs, in place and asynchronous on `stream`: d_f0 / d_f1 [B][cap][259], the match lists airfe_match_lightglue_batch_dev
 * writes (d_idx [B][mcap][2], d_score [B][mcap], d_nmatch [B]; mcap <= 1024), d_F [B][9] or NULL.  d_n0 / d_n1 are the feature counts (not read: the
 * indices come from the matcher). */
int airfe_fundamental_ransac_batch_dev(airfe_ctx* ctx, const float* d_f0, const int* d_n0, const float* d_f1, const int* d_n1, int B, int cap,
                                       int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, double* d_F, void* stream);
/* ≙ the `outlier_rejection` argument at the reference's call sites that pass `true` (map_builder.cc:101 and :96): on = 1 filters the temporal list of
 * airfe_track_frame and the track_* list of airfe_stereo_keyframe_tracked on the device before they are copied back.  Default 0. */
int airfe_set_outlier_rejection(airfe_ctx* ctx, int on);

/* ---- PnP RANSAC: SolvePnPWithCV (src/g2o_optimization/g2o_optimization.cc:1085-1134) ----------------------------------------------------------------
 * The reference seeds every tracked frame's pose (src/map_builder.cc:307-315, on every frame while the IMU is not initialised) and relocalization's best
 * candidate (src/map_user.cc:386-390) with cv::solvePnPRansac(object_points, image_points, K, dist, rvec, tvec, false, 100, 20.0, 0.99, inliers) and the
 * default SOLVEPNP_ITERATIVE.  The contract below restates the PUBLIC behaviour of that call; OpenCV is not part of this project's build or tests, so
 * nothing here is checked against OpenCV and nothing claims bit-equality with it: the numerics are the project's own, on every side — the HIP kernels
 * (airslam_amd/csrc/kernels_pnp.hip), the host core (pnp_solve_host in airslam_amd/csrc/pnp_core.h, which the kernels share) and the numpy restatement
 * (tests/pnp_ref.py).  fp64 unless said otherwise, no fused multiply-adds, sums in the order written; the only non-rational function is sqrt.
 *   input    object points as cv::Point3f (the doubles rounded to float), image points as cv::Point2f, K = (fx, fy, cx, cy) in double, no distortion
 *            (Camera::GetDistCoeffs is all zeros, src/camera.cc:264-266).  Every float is used as a double.
 *   gate     fewer than 8 correspondences (g2o_optimization.cc:1108): count 0, no model.
 *   samples  sample s (0..99) draws attempt a = 0, 1, ... < 64: slot k (0..4) is point floor(hi32(h) * n / 2^32) with
 *            h = splitmix64(0x6A09E667F3BCC909 ^ (s << 32 | a << 8 | k)) (splitmix64 as in "F-matrix RANSAC").  An attempt that repeats an index is
 *            rejected; a sample whose 64 attempts are all rejected yields no model.  No other degeneracy test (OpenCV's PnP callback has no checkSubset).
 *            The draws depend on (s, a, k, n) only.
 *   Jacobi   (used three times below) cyclic Jacobi on a symmetric n x n matrix A, V = I: before each sweep (at most 30) stop when
 *            sum_{p<q} A_pq^2 <= 1e-30 sum_p A_pp^2 (both sums row-major); a sweep visits (p, q) for p = 0..n-2, q = p+1..n-1, skips A_pq == 0, else
 *            th = (A_qq - A_pp) / (2 A_pq), t = sign(th) / (|th| + sqrt(th^2 + 1)) (sign(0) = +1), c = 1 / sqrt(t^2 + 1), s = t c;
 *            A_pp -= t A_pq, A_qq += t A_pq, A_pq = A_qp = 0, for k != p, q: A_kp = A_pk = c A_kp - s A_kq, A_kq = A_qk = s A_kp + c A_kq (old values),
 *            for every k: V_kp = c V_kp - s V_kq, V_kq = s V_kp + c V_kq.  Eigenvalue i = A_ii, eigenvector = column i of V; eigenvalues are ranked by
 *            value, ties by index.
 *   EPnP     (Lepetit, Moreno-Noguer & Fua 2009) on the sample's 5 points:
 *            control points: c0 = the centroid (sum / 5); the 3 x 3 scatter S = sum (X - c0)(X - c0)^T by Jacobi; axis j = 0, 1, 2 = eigenvectors u_j in
 *            descending eigenvalue order, s_j = sqrt(max(lambda_j, 0) / 5), c_{j+1} = c0 + s_j u_j.
 *            alphas: the pseudo-inverse of [s_j u_j]: alpha_{j+1} = u_j . (X - c0) / s_j where s_j > 1e-10 s_0, else 0; alpha_0 = 1 - a1 - a2 - a3.
 *            So PLANAR and COLLINEAR samples are defined (their short axes get weight 0); they give a finite model or none.
 *            M^T M (12 x 12) summed over the points of the rows [a_j fx, 0, a_j (cx - u)] and [0, a_j fy, a_j (cy - v)] (j = 0..3), upper triangle, then
 *            mirrored; its null space = the eigenvectors v_0..v_3 of the 4 smallest eigenvalues (Jacobi), v_0 the smallest.
 *            L (6 x 10) and rho (6) over the control-point pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), d_k = v_k[a] - v_k[b]:
 *            [d0.d0, 2 d0.d1, d1.d1, 2 d0.d2, 2 d1.d2, d2.d2, 2 d0.d3, 2 d1.d3, 2 d2.d3, d3.d3], rho = |c_a - c_b|^2.
 *            betas N = 1: columns (0, 1, 3, 6) of L, least squares -> x; b0 = sqrt(|x0|), b_k = sign(x0) x_k / b0.  N = 2: columns 0..2;
 *            b0 = sqrt(|x0|), b1 = sqrt(|x2|) where x2 has x0's sign (else 0), b0 negated where x1 < 0, b2 = b3 = 0.  N = 3: columns 0..4, as N = 2 and
 *            b2 = x3 / b0.  Each then 5 Gauss-Newton steps on the 4 betas (rows [2 l0 b0 + l1 b1 + l3 b2 + l6 b3, l1 b0 + 2 l2 b1 + l4 b2 + l7 b3,
 *            l3 b0 + l4 b1 + 2 l5 b2 + l8 b3, l6 b0 + l7 b1 + l8 b2 + 2 l9 b3], residual rho - L . b~); a failed solve ends them.  Least squares = the
 *            normal equations by Gaussian elimination with partial pivoting (first largest |pivot|; a pivot not > 0 fails the solve: that N is skipped).
 *            R, t: control points in the camera frame c~_j = sum_k b_k v_k[j], points p_i = sum_j alpha_ij c~_j, all negated when p_0.z < 0; Horn's
 *            quaternion: S = sum (X - X0)(p - p0)^T, the 4 x 4 matrix N(S) of Horn (1987), its eigenvector of the largest eigenvalue (Jacobi)
 *            normalised = q -> R, t = p0 - R X0.  The solution with the smallest summed reprojection distance over the 5 points wins (N = 1 first on
 *            ties); a non-finite model counts as no model.
 *   error    per correspondence: Xc = R X + t; 1/z = 1 where z == 0 (as cvProjectPoints2); u = x / z * fx + cx rounded to float; err = dx^2 + dy^2 in
 *            float without FMA.  Inlier: err <= 400.0f (20 px).
 *   RANSAC   sequentially in sample order: a model replaces the best only with STRICTLY more inliers than max(best, 4); the first wins ties; each
 *            replacement sets niters = RANSACUpdateNumIters(0.99, (n - good) / n, 5, niters) ((1 - ep)^5 as repeated products; log; rint); the search
 *            stops at the first sample index >= niters, 100 samples at most.  The device scores the samples in parallel; one lane then walks the
 *            scores in this order and selects exactly the model the rule selects.
 *   refine   Levenberg-Marquardt on the winner's inliers from the winner (cvFindExtrinsicCameraParams2's 20 iterations, FLT_EPSILON): the update
 *            (w, tau) maps R, t to Cay(w) R, t + tau, Cay(w) = I + 2 / (1 + w.w) ([w]x + [w]x^2) (rational: no trigonometry).  Residuals in double
 *            (u - u_obs); J^T J, J^T r and r^T r are summed as 64 partials (partial l over the points l, l + 64, ... in order) added in lane order.
 *            lambda = 1e-3; each iteration solves (A + lambda diag(A)) delta = -g (Gaussian elimination; a failed solve stops); a trial with a smaller
 *            cost is taken (lambda / 10; stop when max |delta| < FLT_EPSILON), otherwise lambda * 10.  No refinement when the start cost is not finite
 *            and > 0; a non-finite result keeps the RANSAC model.  The inlier mask and count are the RANSAC winner's, as OpenCV reports them.
 *   output   Twc (16 doubles, row-major) as SolvePnPWithCV converts the pose: Rwc = Rcw^T, twc = Rwc (-tcw); Rt (optional) = Rcw row-major, tcw;
 *            inlier [n] (uint8), count.  No model: count 0, identity pose, every mask entry 0.
 * Per problem the batch, the one-call and the host core give the same bytes, whatever the batch size and the problem's position in it. */
/* ≙ cv::solvePnPRansac inside SolvePnPWithCV on ONE problem through host buffers: obj [n][3], img [n][2] doubles, K = (fx, fy, cx, cy); n <= 1024.
 * Twc [16], Rt [12] (may be NULL), inlier [n], *count. */
int airfe_pnp_ransac(airfe_ctx* ctx, const double* obj, const double* img, int n, const double* K, double* Twc, double* Rt, uint8_t* inlier, int* count);
/* the same over B device-resident problems, asynchronous on `stream`: d_obj [B][ncap][3], d_img [B][ncap][2] floats, d_n [B] (clamped to 0..ncap),
 * ncap <= 1024; K is a HOST array read at the call; d_Twc [B][16], d_Rt [B][12] or NULL, d_inlier [B][ncap] (every entry written), d_count [B]. */
int airfe_pnp_ransac_batch_dev(airfe_ctx* ctx, const float* d_obj, const float* d_img, const int* d_n, int B, int ncap, const double* K, double* d_Twc,
                               double* d_Rt, uint8_t* d_inlier, int* d_count, void* stream);

/* ---- Stereo points: Frame::AddRightFeatures (src/frame.cc:141-172) + Frame::BackProjectPoint / Camera::BackProjectStereo (src/frame.cc:299-305,
 * src/camera.cc:275-280) on the stereo match list ----------------------------------------------------------------------------------------------------
 *   cam [8] = min_x_diff, max_x_diff, max_y_diff, bf, fx, fy, cx, cy (HOST array).  Per list entry (left i, right r), in list order: dx = |xl - xr|,
 *   dy = |yl - yr| (float differences, then double); kept when dx > min_x_diff, dx < max_x_diff, dy <= max_y_diff (:147-157); then
 *   parallax = (double)(xl - xr) (a FLOAT difference) must lie in (min_x_diff, max_x_diff) (:161-172); such an entry counts as good and sets
 *   u_right[i] = xr, depth[i] = bf / parallax — a later entry overwrites an earlier one.  The point of a left keypoint with a u_right:
 *   ((xl - cx) / fx', (yl - cy) / fy', 1) * d with 1 / fx' = 1.0 / fx (Camera's _fx_inv) and d = bf / (xl - u_right) in DOUBLE (camera.cc:277): the
 *   two roundings can differ in the last bits, as the reference's do.  Unset keypoints: u_right = depth = -1, point NaN.
 *   *good / d_good = the number of good entries (= airfe_seq_good_stereo_points on the same input). */
int airfe_stereo_points(airfe_ctx* ctx, const double* cam, const float* featL, int nL, const float* featR, int nR, const int32_t* idx, int m, double* u_right,
                        double* depth, double* xyz, int* good);
/* over B device frames: d_featL / d_featR [B][cap][259] (cap <= 4096), d_nL / d_nR [B], d_idx [B][mcap][2] (left, right) + d_nmatch [B] (the stereo
 * matcher's lists); d_u_right / d_depth [B][cap], d_xyz [B][cap][3] (every slot written), d_good [B].  Asynchronous on `stream`. */
int airfe_stereo_points_batch_dev(airfe_ctx* ctx, const double* cam, const float* d_featL, const int* d_nL, const float* d_featR, const int* d_nR, int B,
                                  int cap, const int32_t* d_idx, const int* d_nmatch, int mcap, double* d_u_right, double* d_depth, double* d_xyz,
                                  int* d_good, void* stream);
/* ---- Stereo lines: the loop of Frame::AddRightFeatures over the line matches (src/frame.cc:185-191) and, per valid stereo pair, what
 * Map::InsertKeyframe does with it (src/map.cc:81-95): Frame::TriangulateStereoLine -> TriangulateByStereo (src/line_processor.cc:196-245) with
 * Camera::BackProjectStereo (src/camera.cc:268-280), then Mapline::SetEndpoints -> ComputeLine3DFromEndpoints (src/mapline.cc:74-83,
 * src/line_processor.cc:312-326) ---------------------------------------------------------------------------------------------------------------------
 * One statement for the host entry and the kernel: airslam_amd/csrc/stereoline_core.h (restated in tests/stereoline_ref.py).  Doubles only, no fused
 * multiply-adds, sums in the order written; the only non-rational function is sqrt.  Inputs are finite; a non-finite coordinate never indexes memory and
 * its outputs are unspecified.
 *   input     cam [8] = min_x_diff, max_x_diff, max_y_diff, bf, fx, fy, cx, cy (HOST array, the layout of "Stereo points"; max_y_diff is unused here);
 *             lines [.][4] doubles (x1, y1, x2, y2); line_matches [nL] = airfe_match_lines' output for the stereo pair; Twc [16] row-major, NULL = no
 *             transform: the endpoints stay in the camera frame and nothing is multiplied (an explicit identity pose gives the same VALUES; the sign
 *             of a zero may differ, since (+0 + -0) + t is not -0 + nothing: NULL promises the untouched camera-frame numbers).
 *   select    for left line i: r = line_matches[i]; valid iff r > 0 && r < nR.  The `> 0` is the reference's (frame.cc:186): a match to right line 0
 *             is DROPPED there, and here.  STATED DIFFERENCE: an index >= nR (stale, hostile) counts as invalid and never indexes memory; the
 *             reference would read past its vector.  lines_right_sel[i] = the right line's four doubles, or four zeros when invalid (the reference
 *             leaves the slot unspecified); right_valid[i] = 1 / 0.
 *   gates     dx = x2 - x1, dy = y2 - y1; horizontal iff |dy| <= 3 || |dy / dx| < t, t = 0x1.6a1aa2e1bef6fp-3, first the left line, then the
 *             right.  t is the smallest double whose atan is >= 0.175: the reference's |atan(dy / dx)| < 0.175 without an atan that two libms would
 *             evaluate.  dx == 0 gives +-inf, which passes as atan(+-inf) = +-pi/2 does; dx == dy == 0 is already horizontal by |dy| <= 3.
 *   disparity k = dx_right / dy_right; xr1 = x21 + k * (y11 - y21), xr2 = x21 + k * (y12 - y21); d1 = x11 - xr1, d2 = x12 - xr2; rejected iff
 *             d < min_x_diff || d > max_x_diff on either end (strict: a disparity ON the band passes).
 *   points    fx_inv = 1.0 / fx, fy_inv = 1.0 / fy; p = (((x - cx) * fx_inv) * d, ((y - cy) * fy_inv) * d, 1.0 * d), d = bf / (x - xr); with Twc each
 *             row is ((r0 * px + r1 * py) + r2 * pz) + t.  endpoints = (p1, p2).
 *   line      l = p2 - p1; |l| = sqrt((lx lx + ly ly) + lz lz); |l| < 0.01: no line.  Otherwise d = l / |l| per component, s = (dx p1x + dy p1y) +
 *             dz p1z, p = p1 - d * s, q = p + d, w = p x q = (py qz - pz qy, pz qx - px qz, px qy - py qx); plucker = (w, d).  This is
 *             g2o::Line3D::fromCartesian as published; g2o is not part of this project's build or tests, so nothing here is checked against g2o and
 *             nothing claims equality with it: the formula written here is the contract, on every side.
 *   status    0 map line: endpoints and plucker set | 1 no right line | 2 left line horizontal | 3 right line horizontal | 4 a disparity outside
 *             the band | 5 triangulated but shorter than 0.01: endpoints set, plucker NaN (the reference's SetEndpoints then keeps NEITHER: it
 *             returns before it stores the endpoints, mapline.cc:76).  endpoints / plucker are NaN wherever they are not set.
 *   count [3] valid right lines, lines with status 0 or 5, lines with status 0 (integer sums: the same bytes in every run).
 * Every slot of the first nL lines is written, nothing behind them is touched.  Per frame the batch and the host entry give the same bytes. */
/* ONE frame through host buffers, no device work: lines_left [nL][4], lines_right [nR][4], line_matches [nL], Twc [16] or NULL ->
 * lines_right_sel [nL][4], right_valid [nL], status [nL], endpoints [nL][6], plucker [nL][6], count [3]. */
int airfe_stereo_lines(airfe_ctx* ctx, const double* cam, const double* lines_left, int nL, const double* lines_right, int nR, const int32_t* line_matches,
                       const double* Twc, double* lines_right_sel, uint8_t* right_valid, int32_t* status, double* endpoints, double* plucker,
                       int32_t* count);
/* over B device frames, asynchronous on `stream`, nothing allocated: d_lines_left / d_lines_right [B][capL][4] + d_nlines_left / d_nlines_right [B]
 * (clamped to 0..capL) — the two halves of airfe_stereo_plnet_batch_dev's d_lines [2B][capL][4] / d_nlines [2B], IN PLACE; d_line_matches [B][capL]
 * (airfe_match_lines_batch_dev); d_Twc [B][16] or NULL; B <= 65535.  d_lines_right_sel [B][capL][4], d_right_valid [B][capL] u8, d_status [B][capL] i32,
 * d_endpoints / d_plucker [B][capL][6], d_count [B][3] i32. */
int airfe_stereo_lines_batch_dev(airfe_ctx* ctx, const double* cam, const double* d_lines_left, const int* d_nlines_left, const double* d_lines_right,
                                 const int* d_nlines_right, int capL, const int32_t* d_line_matches, const double* d_Twc, int B, double* d_lines_right_sel,
                                 uint8_t* d_right_valid, int32_t* d_status, double* d_endpoints, double* d_plucker, int32_t* d_count, void* stream);
/* Composite: the line half of a stereo keyframe, from feature rows to map lines, on one stream: AssignPointsToLines on the left frame (frame.cc:125) and
 * on the right (:177), MatchLines on the stereo list with the disparity band cam[0..2] (:147-160, :184) — the three through
 * airfe_assign_points_to_lines_batch_dev / airfe_match_lines_batch_dev as they are — then airfe_stereo_lines_batch_dev.  The CSR relations
 * (d_row_ptr* [B][capL + 1], d_pt_idx* / d_pt_dist* [B][capE], d_total* [B] or NULL) and d_line_matches [B][capL] are the CALLER's, with the shapes of
 * those entries: the left relation stays for the temporal MatchLines of the next frame.  d_featL / d_featR [B][cap][259], d_nL / d_nR [B], d_idx
 * [B][mcap][2] + d_nmatch [B].  Equal, byte for byte, to the four steps done one at a time.  The composite has no memory of its own and the
 * triangulation allocates nothing; the two existing entries keep their own rule: their scratch blocks in the context (line counts [B][capL]; bit rows
 * and row maxima [B][capL][(mcap + 31) / 32]) grow on the first call and on a larger shape, behind a synchronisation of the stream — a call at a shape
 * already seen allocates and synchronises nothing. */
int airfe_stereo_line_landmarks_batch_dev(airfe_ctx* ctx, const double* cam, const double* d_lines_left, const int* d_nlines_left, const double* d_lines_right,
                                          const int* d_nlines_right, int capL, const float* d_featL, const int* d_nL, const float* d_featR, const int* d_nR,
                                          int cap, const int32_t* d_idx, const int* d_nmatch, int mcap, const double* d_Twc, int B, int32_t* d_row_ptrL,
                                          int32_t* d_pt_idxL, double* d_pt_distL, int* d_totalL, int32_t* d_row_ptrR, int32_t* d_pt_idxR, double* d_pt_distR,
                                          int* d_totalR, int capE, int32_t* d_line_matches, double* d_lines_right_sel, uint8_t* d_right_valid,
                                          int32_t* d_status, double* d_endpoints, double* d_plucker, int32_t* d_count, void* stream);
/* Tracking composite: SolvePnPWithCV as tracking feeds it right after a keyframe (map_builder.cc:307-315), all on the device.  Per problem: the
 * keyframe's points d_xyz [B][capK][3] (airfe_stereo_points_batch_dev), the current rows d_feat [B][cap][259], the temporal list d_tidx [B][mcap][2]
 * = (keyframe index, current index) + d_ntrack [B] (airfe_track_frame / the batch matcher; mcap <= 1024).  Correspondences = the list entries whose
 * keyframe point exists, in list order (as SolvePnPWithCV skips null mappoints): object point = the keyframe point rounded to float, image point = the
 * current row's (x, y).  Result: the current frame's pose in the keyframe's camera frame (d_Twc [B][16], d_Rt [B][12] or NULL), d_mask [B][mcap]
 * indexed by LIST ENTRY (0 for entries without a point), d_count [B]. */
int airfe_track_pose_batch_dev(airfe_ctx* ctx, const double* K, const double* d_xyz, int capK, const float* d_feat, int cap, const int32_t* d_tidx,
                               const int* d_ntrack, int mcap, int B, double* d_Twc, double* d_Rt, uint8_t* d_mask, int* d_count, void* stream);

/* ---- Frame optimisation: the vision-only, points-only FrameOptimization of tracking (src/map_builder.cc:353-417 ->
 * src/g2o_optimization/g2o_optimization.cc:446-898) ----------------------------------------------------------------------------------------------------
 * In TrackFrame the line constraint vectors stay empty and, while the IMU is not initialised, there is one free pose and no IMU edge: the call is a
 * pose-only Levenberg-Marquardt over <= 1024 mono / stereo reprojection edges with Huber kernels, three rounds of optimize(10), and a chi-square
 * classification after each round.  The contract below restates the PUBLIC behaviour of that call; g2o is not part of this project's build or tests, so
 * nothing here is checked against g2o and nothing claims equality with it: the numerics are the project's own, on every side — the HIP kernel
 * (airslam_amd/csrc/kernels_poseopt.hip), the host core (poseopt_solve_host in airslam_amd/csrc/poseopt_core.h, which the kernel shares) and the Python
 * restatement (tests/poseopt_ref.py).  fp64, no fused multiply-adds, sums in the order written; the only non-rational function is sqrt.
 *   input    n <= 1024 constraints in list order: map point X (3 doubles, in the frame the start pose is expressed in), observation (x, y, u_right);
 *            STEREO iff u_right > 0 (map_builder.cc:370).  cam = (fx, fy, cx, cy, bf).  Tcb = Rcb (row-major), tcb; NULL = identity.
 *            thr = (mono_point, stereo_point): the chi-square values of `optimization.tracking`; Huber delta = sqrt(threshold)
 *            (g2o_optimization.cc:572-573); information = identity.  Start pose Twc0 (16 doubles, row-major).
 *   state    as VIPose: Rwb = Rwc Rcb, twb = Rwc tcb + twc; Rcw = Rcb Rwb^T, tcw = tcb - Rcw twb; tbc = -(Rcb^T tcb).
 *   edge     Xc = Rcw X + tcw; iz = 1.0 / Xc.z; u = Xc.x iz fx + cx, v = Xc.y iz fy + cy; e = (x - u, y - v) and, stereo, u_right - (u - bf iz)
 *            (edge_project_point.cc:23-44, 100-122); a mono edge's third component is +0.  chi2 = (e0 e0 + e1 e1) + e2 e2.
 *   Jacobian analytic — the one the reference carries in comments (edge_project_point.cc:57-83, 135-166): J = P Rcb D, P = [fx iz, 0, -(fx (Xc.x iz) iz);
 *            0, fy iz, -(fy (Xc.y iz) iz)], stereo third row = the first with (2,2) + bf (iz iz); Xb = Rcb^T Xc + tbc; D = [ -[Xb]x | I ].  A mono
 *            edge's third row is zero.  STATED DIFFERENCE: the reference leaves linearizeOplus to g2o's numeric differentiation.
 *   robust   g2o's Huber: chi2 <= delta^2: rho = chi2, w = 1; else s = sqrt(chi2), rho = 2 s delta - delta^2, w = delta / s.  Per edge of level 0:
 *            H += w J^T J (21 upper entries), g += w J^T e (b = -g), chi += rho.
 *   sums     H, g and chi are summed as 64 partials (partial l over the constraints l, l + 64, ... in order, from +0) added in lane order from +0 —
 *            the rule of the PnP refinement.  The partial count is part of the contract.
 *   optimize g2o's OptimizationAlgorithmLevenberg::solve as published, 10 iterations.  Iteration 0: lambda = 1e-5 max_j |H_jj|, ni = 2.  Each
 *            iteration: H, g, chi at the current pose; then trials: solve (H + lambda I) dx = b by Gaussian elimination with partial pivoting (the
 *            one of "PnP RANSAC"; a failed solve: dx = 0, chi_new = +inf); trial Rwb' = Rwb Cay(dr / 2), twb' = twb + Rwb dt (dr = dx[0..2],
 *            dt = dx[3..5]; Cay as in "PnP RANSAC" — STATED DIFFERENCE: VIPose::Update uses SO3Exp, with which Cay(dr / 2) agrees to second order; no
 *            NormalizeRotation); chi_new = the robust chi at the trial; rho = (chi - chi_new) / (sum_j dx_j (lambda dx_j + b_j) + 1e-3).
 *            rho > 0 and chi_new finite: the trial is taken, lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), ni = 2; else lambda *= ni, ni *= 2
 *            (lambda not finite ends the trials at once).  Trials repeat while rho < 0 and fewer than 10 were made in this iteration.  The round's
 *            optimisation ends early when an iteration made 10 trials, when rho == 0, or when lambda is not finite.
 *   rounds   three times (g2o_optimization.cc:726-814): reset the pose to the START pose, optimize over the level-0 edges, then for EVERY edge
 *            chi2 at the round's final pose, rounded to float: outlier (level 1) iff (double)(float)chi2 > threshold, inlier (level 0) otherwise
 *            — an edge can come back.  n < 10 stops after the first round.  STATED DIFFERENCE: g2o leaves stale errors on inlier edges when the
 *            last trial was rejected; here every edge is evaluated at the accepted pose.
 *   output   Twc = Twb Tcb^-1 (16 doubles), Rt (optional) = Rcw row-major, tcw; inlier [n] (the last round's flags), num_inliers = n - outliers of
 *            the last round (:897).  n == 0, or a final pose that is not finite: Twc = the start pose's 16 doubles, Rt = the start pose's, every
 *            flag 0, num_inliers 0.  A NaN in Rt is written as the canonical quiet NaN (0x7ff8000000000000).
 * Per problem the batch, the one-call and the host core give the same bytes, whatever the batch size and the problem's position in it. */
/* ONE problem through host buffers: X [n][3], obs [n][3] doubles, cam [5], Tcb [12] or NULL, thr [2], Twc0 [16]; n <= 1024.
 * Twc [16], Rt [12] (may be NULL), inlier [n], *num_inliers. */
int airfe_frame_optimize(airfe_ctx* ctx, const double* X, const double* obs, int n, const double* cam, const double* Tcb, const double* thr,
                         const double* Twc0, double* Twc, double* Rt, uint8_t* inlier, int* num_inliers);
/* the same over B device-resident problems, asynchronous on `stream`, no host synchronisation: d_X [B][ncap][3], d_obs [B][ncap][3] doubles, d_n [B]
 * (clamped to 0..ncap), ncap <= 1024, d_Twc0 [B][16]; cam, Tcb (or NULL), thr are HOST arrays read at the call; d_Twc [B][16], d_Rt [B][12] or NULL,
 * d_inlier [B][ncap] (every entry written), d_num [B]. */
int airfe_frame_optimize_batch_dev(airfe_ctx* ctx, const double* d_X, const double* d_obs, const int* d_n, int B, int ncap, const double* d_Twc0,
                                   const double* cam, const double* Tcb, const double* thr, double* d_Twc, double* d_Rt, uint8_t* d_inlier, int* d_num,
                                   void* stream);
/* Tracking composite: FramePoseOptimization without IMU (map_builder.cc:307-317, 353-417) on the inputs of airfe_track_pose_batch_dev, all on the
 * device, nothing copied to the host in between.  Additional inputs: d_u_right [B][cap] of the CURRENT frame (NULL = every constraint mono, the
 * normal-frame case; for a keyframe it is airfe_stereo_points_batch_dev's output), d_Twc_last [B][16] (the last tracked pose; NULL = identity),
 * lost_num_match, cam = (fx, fy, cx, cy, bf), thr.  Per problem: (1) the gather and PnP RANSAC of airfe_track_pose_batch_dev; (2) the seed is the PnP
 * pose, or Twc_last when |t_pnp - t_last| > 1.0 or the PnP count < lost_num_match; (3) constraints = the list entries whose keyframe point exists, in
 * list order: X = the keyframe point in double, (x, y) = the current row's, u_right = d_u_right[current index] (the matcher's lists are one-to-one; a
 * repeated current index is NOT deduplicated: each entry is a constraint of its own); (4) the frame optimisation from the seed, Tcb = identity.
 * d_Twc [B][16] = the optimised pose when num_inliers > lost_num_match, else the seed; d_Rt [B][12] or NULL likewise; d_mask [B][mcap] by LIST ENTRY =
 * the optimisation's inlier flags (0 for entries without a point; the reference applies them only when d_ok is set); d_num [B] = num_inliers;
 * d_ok [B] = num_inliers > lost_num_match; d_pnp_count [B] or NULL = the PnP count.  Equal, byte for byte, to the steps done one at a time. */
int airfe_track_pose_opt_batch_dev(airfe_ctx* ctx, const double* cam, const double* thr, int lost_num_match, const double* d_xyz, int capK,
                                   const float* d_feat, int cap, const int32_t* d_tidx, const int* d_ntrack, int mcap, int B, const double* d_u_right,
                                   const double* d_Twc_last, double* d_Twc, double* d_Rt, uint8_t* d_mask, int* d_num, int* d_ok, int* d_pnp_count,
                                   void* stream);

/* ---- next row after the path ---------------------------------------------------- */
/* ≙ AssignPointsToLines (src/line_processor.cc:68-120), called on the path's own outputs (frame.cc:125,177,184).
 *   lines [L][4] doubles (x1,y1,x2,y2) = the std::vector<Eigen::Vector4d> storage; feat [N][259] rows (x,y = floats 1,2).
 *   Result in CSR form: row_ptr [L+1]; for line i the entries row_ptr[i] .. row_ptr[i+1]-1 of pt_idx / pt_dist are the
 *   (point index, distance) pairs of relation[i] in ascending point index = the iteration order of its std::map<int,double>.
 *   cap = capacity of pt_idx / pt_dist; *total = row_ptr[L]; fails (and writes nothing past cap) if total > cap. */
int airfe_assign_points_to_lines(airfe_ctx* ctx, const double* lines, int L, const float* feat, int N, int32_t* row_ptr,
                                 int32_t* pt_idx, double* pt_dist, int cap, int* total);

/* ≙ MatchLines (src/line_processor.cc:122-172), called right after the point matcher on two frames' relations (frame.cc:177-190).
 *   (row_ptr0, pt_idx0) / (row_ptr1, pt_idx1): the CSR relations of airfe_assign_points_to_lines for frame 0 / frame 1 (L0 / L1 lines,
 *   point_num0 / point_num1 keypoints); matches [M][2] = (queryIdx, trainIdx) of the cv::DMatch list.
 *   line_matches [L0]: index of the matched line of frame 1 or -1 (all -1 when any of the four counts is 0, :132). */
int airfe_match_lines(airfe_ctx* ctx, const int32_t* row_ptr0, const int32_t* pt_idx0, int L0, int point_num0, const int32_t* row_ptr1,
                      const int32_t* pt_idx1, int L1, int point_num1, const int32_t* matches, int M, int32_t* line_matches);

/* ---- the step AFTER the path: BoW quantisation of the descriptors ------------------------------------------ */
/* ≙ the vocabulary Database's constructor loads (src/bow/database.cc; voc/point_voc_L4.bin is absent from the reference checkout):
 *   the tree of TemplatedVocabulary (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:298-323) flattened so that the children of
 *   node i are the n_children[i] consecutive nodes from first_child[i] on (0 children = leaf = word); node 0 is the root;
 *   node_desc [n_nodes][256] floats, word_id / weight per node (meaningful at leaves). */
int airfe_bow_load(airfe_ctx* ctx, const float* node_desc, const int32_t* first_child, const int32_t* n_children, const int32_t* word_id,
                   const double* weight, int n_nodes);
/* ≙ the loop of Database::FrameToBow (src/bow/database.cc:66-84): TemplatedVocabulary::transform(feature, id, w) (…Vocabulary.h:1313-1352)
 *   for each of the N feature rows [N][259]: word_of_features[i] = leaf word id, or UINT_MAX where the leaf weight is <= 0;
 *   weight_of_features[i] = w (may be NULL).  bow_vector.addWeight / normalize: airfe_bow_vector below; word_features (std::map work) stays reference code. */
int airfe_bow_transform(airfe_ctx* ctx, const float* feat, int N, uint32_t* word_of_features, double* weight_of_features);
int airfe_bow_transform_dev(airfe_ctx* ctx, const float* d_feat, int N, uint32_t* d_word, float* d_weight, void* stream);

/* ---- BoW keyframe database: the link in front of the matcher in MapUser::Relocalization (src/map_user.cc:106-390) and MapRefiner::LoopDetection
 * (src/map_refiner.cc:95-235) ---------------------------------------------------------------------------------------------------------------------------
 *   Detect -> Database::FrameToBow -> Database::Query -> sharing-word filter -> Database::Score (L1) -> grouping -> top 3 / 5 candidates
 *          -> MatchingPoints(query, candidate, matches, true) per candidate -> the candidate with the most matches -> SolvePnPWithCV
 * RESTATED here, on the device, bit for bit (DBoW2 compiled unchanged is the test's reference for the vector; tests/bowdb_ref.py restates the rest):
 * FrameToBow to its end, AddFrame, Query, the two callers' filters, L1Scoring::score, the best-candidate rule — and, in the block "Grouping" below, the
 * GROUPING between the scores and the candidates (map_user.cc:177-264, map_refiner.cc:132-211) over a covisibility table the caller hands to the
 * database (airfe_bowdb_attach_map / airfe_bowdb_set_covisibility) or builds there from the frames' map-point ids (the block "Map-point ids and the
 * covisibility build" below).  Relocalisation's junction term, which enters the grouping as one number per frame (d_extra), is computed on the device by
 * the block "Junction term" below.  The candidate list below IS the reference's frame_scores map.  airfe_bowdb_topk_dev is the PROJECT'S OWN ranking for callers without a
 * covisibility graph, not the reference's grouping.  Every floating-point sum is sequential in the order given; no fused multiply-adds.
 *   vector   Database::FrameToBow (src/bow/database.cc:57-89): per feature the descent of airfe_bow_transform (the same kernel); a feature counts iff its
 *            word's weight is > 0 (word_of_features = UINT_MAX otherwise).  The weights are the vocabulary's doubles (WordValue).  BowVector::addWeight:
 *            one entry per distinct word, its weights added in ascending feature index, in double.  BowVector::normalize(L1): tot = the sum of |v| in
 *            ascending word id, from +0; every v / tot (a division).  Output in ascending word id, nw entries; rows beyond nw are not written; a frame
 *            whose every word is stopped, or with no feature, gives nw = 0.
 *   add      Database::AddFrame (:98-106): a frame's handle is its insertion index (0, 1, ...), which the caller maps to its FramePtr.
 *   sharing  sharing[q][f] = the number of words present in both vectors = what Database::Query (:108-120) leaves in frame_sharing_words[f]
 *            (a frame with 0 is absent from that map and never a candidate).
 *   filter   max_sharing[q] over ALL frames, before any other test (map_user.cc:142-145, map_refiner.cc:104-107);
 *            thr = max((int)(max_sharing * ratio), min_words) with the product in float32, truncated (ratio 0.3f at map_user.cc:146, 0.5f at
 *            map_refiner.cc:108; min_words 8).  Frame f is a candidate iff sharing >= thr and (d_max_index == NULL or f < d_max_index[q]:
 *            map_refiner.cc:115's GetFrameId() >= frame_id) and (d_exclude == NULL or bit f of row q clear: the covisible frames of :115, a bit row of
 *            exclude_words 32-bit words per query supplied by the caller; frames past the row are not excluded).
 *   score    L1Scoring::score(v1 = the FRAME's vector, v2 = the QUERY's) as map_user.cc:165 passes them (3rdparty/DBoW2/src/ScoringObject.cpp:23-68):
 *            s = +0; over the common words in ascending word id s += (fabs(v1 - v2) - fabs(v1)) - fabs(v2); score = -s / 2.0 (so two vectors without a
 *            common word score -0.0).  The argument order matters to the last bit.
 *   output   per query the candidates in ascending frame index — frame, sharing, score — up to ccap; d_ncand[q] = the full count (may exceed ccap:
 *            the first ccap are written, entries past the count are not written); d_max_sharing[q].
 *   best     map_user.cc:360-376 / map_refiner.cc:213-230: the candidates in the GIVEN order, each through MatchingPoints(query, candidate, ...,
 *            outlier_rejection); a candidate replaces the best only with a STRICTLY longer list, starting from an empty one: the first of equals
 *            wins, a candidate with 0 matches never does.
 * A database belongs to one context (its stream rules apply) and must be destroyed before it.  Capacity errors are return codes. */
typedef struct airfe_bowdb airfe_bowdb;
typedef struct airfe_bowdb_filter {
  float ratio;                  /* 0.3f relocalisation, 0.5f loop detection */
  int min_words;                /* 8 */
  const int* d_max_index;       /* DEVICE [Q] or NULL */
  const uint32_t* d_exclude;    /* DEVICE [Q][exclude_words] bit rows (bit f & 31 of word f >> 5) or NULL */
  int exclude_words;
} airfe_bowdb_filter;
/* ONE frame through host buffers: feat [n][259] (n <= 1024); ids / vals [>= n]; *nw; word_of_features [n] or NULL. */
int airfe_bow_vector(airfe_ctx* ctx, const float* feat, int n, uint32_t* ids, double* vals, int* nw, uint32_t* word_of_features);
/* B device frames, asynchronous on `stream`: d_feat [B][cap][259], d_n [B] (clamped to 0..cap), cap <= 1024; d_ids u32 [B][cap], d_vals f64 [B][cap],
 * d_nw [B]; d_word u32 [B][cap] or NULL = word_of_features (only a frame's first n entries mean anything).  A frame's bytes do not depend on B or on
 * its position in the batch. */
int airfe_bow_vector_batch_dev(airfe_ctx* ctx, const float* d_feat, const int* d_n, int B, int cap, uint32_t* d_ids, double* d_vals, int* d_nw,
                               uint32_t* d_word, void* stream);
/* storage: fixed-stride rows [max_frames][cap] of ids / values (+ [max_frames][cap][259] feature rows and counts with keep_features, which the
 * composite needs).  Needs a loaded vocabulary (its word count sizes the query table). */
int airfe_bowdb_create(airfe_ctx* ctx, int max_frames, int cap, int keep_features, airfe_bowdb** out);
int airfe_bowdb_destroy(airfe_bowdb* db);
int airfe_bowdb_clear(airfe_bowdb* db);             /* size = 0; a query already queued must have completed */
int airfe_bowdb_size(const airfe_bowdb* db);        /* frames added; -1 for NULL */
/* B vectors (airfe_bow_vector_batch_dev's outputs, same cap as the database) become frames size .. size + B - 1; d_feat / d_n (the frames' rows and
 * counts) are needed iff keep_features.  Asynchronous on `stream`; a full database is an error and adds nothing. */
int airfe_bowdb_add_batch_dev(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, const float* d_feat, const int* d_n, int B,
                              int cap, void* stream);
int airfe_bowdb_add(airfe_bowdb* db, const uint32_t* ids, const double* vals, const int* nw, const float* feat, const int* n, int B, int cap);   /* host buffers */
/* Q query vectors [Q][cap] against all N = size frames, asynchronous on `stream`, no host synchronisation.  d_cand_frame / d_cand_sharing i32
 * [Q][ccap], d_cand_score f64 [Q][ccap], d_ncand [Q], d_max_sharing [Q]; d_sharing i32 [Q][N] or NULL (the dense counts, for tests). */
int airfe_bowdb_query_batch_dev(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, int Q, int cap,
                                const airfe_bowdb_filter* filter, int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap,
                                int* d_ncand, int* d_max_sharing, int32_t* d_sharing, void* stream);
/* the project's own ranking (NOT the reference's grouping): per query the K <= 8 candidates (of the first min(ncand, ccap)) by descending score, ties
 * to the lower frame index; d_top i32 [Q][K] padded with -1, d_top_score f64 [Q][K] or NULL (0 where padded). */
int airfe_bowdb_topk_dev(airfe_bowdb* db, const int32_t* d_cand_frame, const double* d_cand_score, const int* d_ncand, int Q, int ccap, int K,
                         int32_t* d_top, double* d_top_score, void* stream);
/* "best" above for Q queries x K <= 5 candidates (d_cand i32 [Q][K], -1 or an index past the database = a hole, skipped), on the kept feature rows:
 * the rows are gathered into a [Q K] pair batch, airfe_match_lightglue_batch_dev's code runs on it and, with outlier_rejection,
 * airfe_fundamental_ransac_batch_dev's.  d_qfeat [Q][cap][259] (cap = the database's), d_qn [Q]; d_best [Q] (frame index or -1), the winner's list
 * d_idx [Q][mcap][2] = (query index, candidate index) / d_score [Q][mcap] / d_nmatch [Q] (0 without a winner; entries past the count are not written),
 * d_nmatch_all [Q][K] or NULL (0 for holes).  Q * K above cfg.max_batch is an error.  PnP and the refinement behind it: airfe_relocalize_batch_dev
 * below, on the map points the database holds once airfe_bowdb_attach_map was called (or the entries above, on points the caller holds). */
int airfe_bowdb_match_candidates_batch_dev(airfe_ctx* ctx, airfe_bowdb* db, const float* d_qfeat, const int* d_qn, int Q, int cap, const int32_t* d_cand,
                                           int K, int outlier_rejection, int32_t* d_best, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch,
                                           int* d_nmatch_all, void* stream);

/* ---- Map state in the database (opt-in): what the grouping and the relocalisation composite read ----------------------------------------------------
 * airfe_bowdb_attach_map (needs keep_features) allocates
 *   points        [max_frames][cap][3] f64 in the map's world frame, one per FEATURE ROW of the stored frame, initialised to NaN; NaN (in x) = "no valid
 *                 map point at this row" (the convention of airfe_stereo_points' xyz): the caller writes NaN where mpt == nullptr || !mpt->IsValid().
 *   covisibility  CSR: row_ptr [max_frames + 1], nbr i32 [max_edges], weight i32 [max_edges]; initially empty.  airfe_bowdb_set_covisibility REPLACES the
 *                 whole graph (as Map::UpdateCovisibilityGraph does) from HOST arrays of n_frames rows (frames past n_frames get empty rows); every row
 *                 must be strictly ascending in nbr and row_ptr must start at 0 and not decrease, otherwise the call fails and changes nothing.  The
 *                 table is the reference's _covisibile_frames as it is: it INCLUDES each frame's entry for itself (UpdateFrameCovisibility counts a
 *                 frame among the observers of its own points); the library neither adds nor removes it.  airfe_bowdb_build_covisibility[_dev] ("Map-point ids and the covisibility build" below)
 *                 builds the same table on the device.
 *   positions     [max_frames][3] f64, optional (airfe_bowdb_set_positions, host rows): the keyframes' twc, read by the loop form only.
 * The set_* / get_* entries on host buffers synchronise the context's stream; a grouping queued on ANOTHER stream must have completed before the graph
 * is replaced.  airfe_bowdb_set_points_dev is asynchronous on `stream`. */
int airfe_bowdb_attach_map(airfe_bowdb* db, int max_edges);
int airfe_bowdb_set_points_dev(airfe_bowdb* db, int first_frame, int B, const double* d_xyz, void* stream);   /* d_xyz [B][cap][3] -> frames first_frame .. */
int airfe_bowdb_set_points(airfe_bowdb* db, int first_frame, int B, const double* xyz);                      /* host buffer */
int airfe_bowdb_get_points(airfe_bowdb* db, int first_frame, int B, double* xyz);                            /* host buffer [B][cap][3] */
int airfe_bowdb_set_covisibility(airfe_bowdb* db, const int32_t* row_ptr, const int32_t* nbr, const int32_t* weight, int n_frames);
/* row_ptr [max_frames + 1]; nbr / weight [edge_cap] (may be NULL when the graph is empty); *n_edges = row_ptr[max_frames] (an error when > edge_cap) */
int airfe_bowdb_get_covisibility(airfe_bowdb* db, int32_t* row_ptr, int32_t* nbr, int32_t* weight, int edge_cap, int* n_edges);
int airfe_bowdb_set_positions(airfe_bowdb* db, int first_frame, int B, const double* pos);                   /* host buffer [B][3] */

/* ---- Grouping: between the scores and the candidates of MapUser::Relocalization (src/map_user.cc:177-270, 331, 347-363) and MapRefiner::LoopDetection
 * (src/map_refiner.cc:132-214) ---------------------------------------------------------------------------------------------------------------------
 * Three statements that agree bit for bit: the host routine bowgroup_host (airslam_amd/csrc/bowgroup_core.h), the kernel (kernels_bowgroup.hip, which
 * calls the same header's routines from its lanes) and tests/bowgroup_ref.py.  fp64, every sum sequential in the order written, no fused multiply-adds.
 *   input    per query the candidate list of airfe_bowdb_query_batch_dev: (frame, score) in ascending frame index, the first min(ncand, ccap) entries;
 *            ccap <= 4096 (beyond: a capacity error).  A query whose ncand > ccap gets status 2 (overflow) and no groups.
 *   order    STATED DIFFERENCE: the reference iterates std::map<FramePtr, ...> and std::set<FramePtr> in POINTER order, which is unspecified.  Every such
 *            iteration here is in ascending frame index.
 *   per candidate i, in list order (map_user.cc:183-217 ≡ map_refiner.cc:138-172): score_i = 0 + s_i (group_score starts at 0), deputy = i, deputy_score = s_i; for each covisibility
 *            entry of frame i in ascending neighbour index with weight > 10 whose neighbour is in the candidate list: score_i += s_nbr, and the
 *            neighbour becomes the deputy iff s_nbr > deputy_score (strictly).  The frame's entry for ITSELF is an entry like any other: with a weight
 *            above 10 the frame's own score is added twice, as in the reference.
 *   replacement  sequentially in list order: group i is stored under its deputy iff that deputy has no group yet or its stored group_score < score_i;
 *            best_group_score starts at -1 and is raised by every stored group that exceeds it.  best_group_score < 0: no groups (status 1; a query
 *            without candidates ends here as well).
 *   relocalisation form (mode 0; map_user.cc:221-270, 331, 347-363)
 *            (1) every stored group is re-summed: its members are the stored candidate and its qualifying neighbours, each once; more than 5 members:
 *            the five largest scores added in descending order, otherwise every score in ascending frame index; from +0.  (2) best = the maximum of
 *            the re-summed scores, from 0.0.  (3) with more than 3 groups, those with score < best * 0.5 are dropped.  (4) d_extra (f64 [Q][N],
 *            N = the database's size, or NULL): d_extra[q][deputy] is added to each remaining group's score — the caller's junction term
 *            junction_frame_scores * (1 + rate) of :329-331.  (5) descending score, ties to the lower frame index (std::sort is not stable: the tie
 *            rule is the project's, STATED DIFFERENCE).  (6) the first K <= 3 deputies are the candidates.
 *   loop form (mode 1; map_refiner.cc:176-214)  no re-sum: a group keeps score_i.  (1) groups whose deputy lies farther than d_max_dist[q] from
 *            d_qpos[q] are dropped: sqrt((dx dx + dy dy) + dz dz) in double, dropped iff > d_max_dist[q] (positions: airfe_bowdb_set_positions).
 *            (2) with more than 3 groups LEFT, those with score < best_group_score * 0.5 are dropped — best_group_score is the replacement pass's,
 *            taken before the distance filter, as in the reference.  (3) ranked as above; K <= 5.  d_extra is not read.
 *   output   d_group_frame i32 [Q][K] (the deputies, -1 padded: the shape airfe_bowdb_match_candidates_batch_dev takes as d_cand), d_group_score f64
 *            [Q][K] (0 where padded), d_ngroups [Q] (the groups left after the filters; may exceed K), d_status [Q]: 0 ok, 1 no group, 2 overflow.
 * Asynchronous on `stream`, no host synchronisation; a query's bytes do not depend on Q or on its position in the batch. */
int airfe_bowdb_group_dev(airfe_bowdb* db, int mode, const int32_t* d_cand_frame, const double* d_cand_score, const int* d_ncand, int Q, int ccap, int K,
                          const double* d_extra, const double* d_qpos, const double* d_max_dist, int32_t* d_group_frame, double* d_group_score,
                          int* d_ngroups, int* d_status, void* stream);

/* ---- Relocalisation composite: MapUser::Relocalization from the query's feature rows to the pose (src/map_user.cc:129-460), on one stream, nothing
 * copied to the host in between.  Per query, byte for byte the steps done one at a time through the entries above:
 *   (1) airfe_bow_vector_batch_dev's code; airfe_bowdb_query_batch_dev's with (ratio, min_words) and no other filter, over every stored frame (at most
 *       4096); the grouping in relocalisation form with d_extra; airfe_bowdb_match_candidates_batch_dev's code on the K deputies.
 *   (2) no candidate: stage 1.  No group: stage 2.  nmatch < min_inlier (or no winner): stage 3 (:377).
 *   (3) correspondences = the winner's list entries whose candidate row has a map point (x not NaN) in the database's point table, in list order — the
 *       matcher's lists ascend in query index, SolvePnPWithCV's loop order; a repeated index is not deduplicated.  Object point = the map point rounded
 *       to float, image point = the query row's (x, y).
 *   (4) the PnP RANSAC above with K = cam[0..3]; the pose is PnP's, or the identity without a model.  There is no seed fallback here.
 *   (5) pose_refinement: fewer correspondences than min_inlier: stage 4, the pose stays PnP's, num = 0 and the mask is 0 (:448).  Otherwise the frame
 *       optimisation above from the PnP pose, Tcb = identity, every constraint mono (u_right = -1: the query has no right image); the pose is the
 *       optimised one, num its num_inliers, the mask its flags.  Without pose_refinement num and the mask are PnP's.
 *   (6) num < min_inlier: stage 5 (:460).
 * d_ok [Q]; d_stage [Q] (0 = ok); d_Twc [Q][16] = what the reference's `pose` holds at the return (identity for stages 1 - 3); d_best [Q] (-1 without a
 * winner); d_num [Q] (0 for stages 1 - 4); d_mask [Q][mcap] by LIST ENTRY (every entry written); the winner's list d_idx [Q][mcap][2] = (query index,
 * candidate index) / d_score / d_nmatch as airfe_bowdb_match_candidates_batch_dev writes them; d_pnp_count [Q] or NULL.  mcap <= 1024; Q * K above
 * cfg.max_batch, a database without airfe_bowdb_attach_map and one of more than 4096 frames are errors.  A query's bytes depend neither on Q nor on its
 * position in the batch. */
typedef struct airfe_reloc_cfg {
  float ratio;            /* 0.3f */
  int min_words;          /* 8 */
  int K;                  /* 3 (GoodCandidateNum) */
  int outlier_rejection;  /* 1: MatchingPoints(..., true) */
  int min_inlier;         /* RelocalizationConfig::min_inlier */
  int pose_refinement;    /* whether step 5 runs */
  double cam[5];          /* fx, fy, cx, cy, bf */
  double thr[2];          /* the chi-square values of `pose_estimation`: mono_point, stereo_point */
} airfe_reloc_cfg;
int airfe_relocalize_batch_dev(airfe_ctx* ctx, airfe_bowdb* db, const airfe_reloc_cfg* cfg, const float* d_qfeat, const int* d_qn, int Q, int cap,
                               const double* d_extra, int* d_ok, int* d_stage, double* d_Twc, int32_t* d_best, int* d_num, uint8_t* d_mask, int32_t* d_idx,
                               float* d_score, int mcap, int* d_nmatch, int* d_pnp_count, void* stream);

/* ---- Map state for loop detection (opt-in, allocated by airfe_bowdb_attach_map): what MapRefiner::LoopDetection reads of a loaded map next to the
 * tables above -----------------------------------------------------------------------------------------------------------------------------------------
 *   poses     [max_frames][16] f64 row-major Twc, initialised to the identity.  airfe_bowdb_set_poses (host rows [B][16]) ALSO writes each pose's
 *             translation column into the positions table and marks the positions as set, so one call serves the loop form of the grouping.
 *   u_right   [max_frames][cap] f64, one per FEATURE ROW of the stored frame, initialised to -1.0: the stored frame's _u_right.  A value > 0 means the row
 *             has a right-image match (the convention of "Frame optimisation").
 * Stream and synchronisation rules are those of airfe_bowdb_set_points / _set_points_dev; frames beyond max_frames are a return code and change nothing. */
int airfe_bowdb_set_poses(airfe_bowdb* db, int first_frame, int B, const double* Twc);                       /* host buffer [B][16] */
int airfe_bowdb_get_poses(airfe_bowdb* db, int first_frame, int B, double* Twc);                             /* host buffer [B][16] */
int airfe_bowdb_set_u_right_dev(airfe_bowdb* db, int first_frame, int B, const double* d_u_right, void* stream);   /* d_u_right [B][cap] */
int airfe_bowdb_set_u_right(airfe_bowdb* db, int first_frame, int B, const double* u_right);                 /* host buffer [B][cap] */
int airfe_bowdb_get_u_right(airfe_bowdb* db, int first_frame, int B, double* u_right);                       /* host buffer [B][cap] */

/* ---- Stored queries against their predecessors: the query and the filter of MapRefiner::LoopDetection (src/map_refiner.cc:95-130) for frames that are
 * ALREADY in the database.  The reference walks the keyframes of a loaded map and queries frame fq BEFORE it adds it (:88-89): the database then holds
 * frames 0 .. fq - 1 only.  airfe_bowdb_query_batch_dev on a fully loaded database cannot express that: its max_sharing is taken over every stored frame,
 * frame fq itself (which shares all of its words) and every later frame included, so the threshold comes out wrong even with d_max_index.  Here, for
 * query q with fq = d_qframe[q] (i32 [Q], any order, repeats allowed, Q <= 4096):
 *   query    the stored vector of frame fq, read from the database on the device.
 *   exists   only frames f < fq.  sharing and score as in "BoW keyframe database" (v1 = the stored frame's vector, v2 = the query's, the same order).
 *   thr      max_sharing over f < fq only; thr = max((int)((float)max_sharing * ratio), min_words), the product in float32.
 *   filter   f is a candidate iff f < fq, sharing > 0, sharing >= thr and — with exclude_covisible — f is not a neighbour in row fq of the covisibility
 *            CSR at ANY weight (covi_frames.count(fsw), :115; neighbours >= fq are ignored; needs airfe_bowdb_attach_map).
 *   output   what airfe_bowdb_query_batch_dev writes: the candidates in ascending frame index up to ccap, d_ncand[q] = the full count (may exceed ccap),
 *            d_max_sharing[q]; d_sharing i32 [Q][N] or NULL: the dense counts, 0 at f >= fq.  fq outside 0 .. size - 1: ncand = 0, max_sharing = 0.
 * Three statements that agree bit for bit: loopdet_select_host (airslam_amd/csrc/loopdet_core.h), the kernels (kernels_loopdet.hip around the unchanged
 * query kernel) and tests/loopdet_ref.py.  Asynchronous on `stream`, no host synchronisation; a query's bytes depend neither on Q nor on its position. */
int airfe_bowdb_query_stored_batch_dev(airfe_bowdb* db, const int32_t* d_qframe, int Q, float ratio, int min_words, int exclude_covisible,
                                       int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap, int* d_ncand, int* d_max_sharing,
                                       int32_t* d_sharing, void* stream);

/* ---- Loop detection composite: MapRefiner::LoopDetection (src/map_refiner.cc:65-235) and the pose of RelativatePoseEstimation (:237-320, :327-333) for
 * a list of stored frames, on one stream, nothing copied to the host in between.  Per query q with fq = d_qframe[q], byte for byte the steps done one at
 * a time through the entries above:
 *   (1) airfe_bowdb_query_stored_batch_dev's code with (ratio, min_words) and exclude_covisible = 1.
 *   (2) odom(fq) = the sum over f = 1 .. fq of |pos[f] - pos[f - 1]|, added sequentially in ascending f from +0, each term sqrt((dx dx + dy dy) + dz dz)
 *       in double (:66-81; pos = the positions table, which airfe_bowdb_set_poses fills); max_dist = odom(fq) * distance_rate; qpos = pos[fq].
 *   (3) the grouping in loop form (mode 1) on the candidate list with qpos and max_dist; airfe_bowdb_match_candidates_batch_dev's code on the K <= 5
 *       deputies, the query's feature rows and count being the STORED rows of fq.  The winner b: the first candidate with strictly the longest list.
 *   (4) no candidate: stage 1.  No group: stage 2.  No winner or nmatch <= min_matches: stage 3 (:232 is a strict >).
 *   (5) constraints = the winner's list entries (qi, ci), in list order, whose map point xyz[b][ci] exists (x not NaN): X = xyz[b][ci],
 *       obs = (feat[fq][qi].x, feat[fq][qi].y, u) with u = u_right[fq][qi] if that is > 0, else -1.0.  STATED DIFFERENCE: a repeated index is not
 *       deduplicated (the reference gates on distinct map-point ids, points.size(); the matcher's lists are one-to-one).  Fewer than min_points
 *       constraints: stage 4, none are handed over.
 *   (6) the frame optimisation above from the STORED pose of fq (AddFrameVertex(frame, ...), :262), Tcb = identity.  num < min_inliers: stage 5.
 *   (7) from the optimised Twq and the stored Twl of b, in double, no fused multiply-adds, summed in the order written:
 *       Rlq[i][j] = (Rwl[0][i] Rwq[0][j] + Rwl[1][i] Rwq[1][j]) + Rwl[2][i] Rwq[2][j];  d = twq - twl;  tlq[i] = (Rwl[0][i] d0 + Rwl[1][i] d1) + Rwl[2][i] d2.
 * Every entry is written: d_ok [Q]; d_stage [Q] (0 = ok); d_loop [Q] = b or -1 (as airfe_bowdb_match_candidates_batch_dev's d_best); d_Twq [Q][16] = the
 * stored pose for stages 1 - 4 (the identity for an fq outside the database), the optimised pose for stages 0 and 5; d_Rlq [Q][9] row-major / d_tlq [Q][3]
 * = identity / zero for stages 1 - 4, from the optimised pose for stages 0 and 5; d_num [Q] (0 for stages 1 - 4); d_mask [Q][mcap] = the optimisation's
 * flags by LIST ENTRY (0 where there is no point); the winner's list d_idx [Q][mcap][2] / d_score / d_nmatch as
 * airfe_bowdb_match_candidates_batch_dev writes them; d_ncons [Q] or NULL = the constraints found (0 for stages 1 - 3).
 * Return codes: no map state; poses never set (airfe_bowdb_set_poses); Q * K above cfg.max_batch; mcap > 1024; more than 4096 frames in the database;
 * K outside 1 .. 5; Q > 4096.  A caller with a large map runs the stored query and airfe_bowdb_group_dev over all frames first (both are cheap) and hands
 * the composite only the frames that kept a group, in chunks of max_batch / K: d_qframe is an arbitrary list for that reason.
 * OUT OF SCOPE (the caller's, as in the reference): the "find more matches" search of :322-438, the pose graph, junction sentences.  (TriangulateMappoint
 * and the mappoint merge are the blocks "Map-point triangulation" and "Map-point merge" below.) */
typedef struct airfe_loop_cfg {
  float ratio;            /* 0.5f */
  int min_words;          /* 8 */
  int K;                  /* <= 5 (GoodCandidateNum) */
  int outlier_rejection;  /* 1: MatchingPoints(..., true) */
  double distance_rate;   /* 0.03 (:179) */
  int min_matches;        /* 50: a winner needs STRICTLY more matches (:232) */
  int min_points;         /* 50 (:301) */
  int min_inliers;        /* 50 (:308) */
  double cam[5];          /* fx, fy, cx, cy, bf */
  double thr[2];          /* the chi-square values of map_optimization_config: mono_point, stereo_point */
} airfe_loop_cfg;
int airfe_loop_detect_batch_dev(airfe_ctx* ctx, airfe_bowdb* db, const airfe_loop_cfg* cfg, const int32_t* d_qframe, int Q, int* d_ok, int* d_stage,
                                int32_t* d_loop, double* d_Twq, double* d_Rlq, double* d_tlq, int* d_num, uint8_t* d_mask, int32_t* d_idx, float* d_score,
                                int mcap, int* d_nmatch, int* d_ncons, void* stream);

/* ---- Map-point ids and the covisibility build: Map::UpdateCovisibilityGraph (src/map.cc:1385-1418) for a loaded map, on the device -------------------
 * The table the grouping and the stored query read, from the IDENTITIES of the map points at the stored frames' feature rows.
 * airfe_bowdb_attach_point_ids (needs airfe_bowdb_attach_map; a second attach is a return code) allocates
 *   point_id   i32 [max_frames][cap], one per FEATURE ROW of the stored frame, initialised to -1.  id >= 0: the map point at that row; the caller writes -1
 *              where mpt == nullptr || !mpt->IsValid() — the rows that hold NaN in the point table.
 *   work       8 bytes per point (max_points + 1 entries) and 8 bytes per feature row, in one block that the build never replaces.  max_points is
 *              1 .. 16777216 (2^24: 128 MiB of work memory at the limit); outside that: a return code.  Every build clears and scans the per-point
 *              arrays, so its cost grows with max_points: size it by the map, not by the limit.
 * airfe_bowdb_set_point_ids (host buffer [B][cap]) refuses an id < -1 or >= max_points and changes nothing then; _set_point_ids_dev copies blindly.  Stream
 * and synchronisation rules are those of airfe_bowdb_set_points / _set_points_dev; frames beyond max_frames are a return code and change nothing.
 * THE BUILD.  With size = the frames in the database and n[f] = the stored feature count of frame f (clamped to 0 .. cap):
 *   valid(f, i)   f < size, i < n[f] and 0 <= point_id[f][i] < max_points
 *   obs(m)        { f : some i with valid(f, i) and point_id[f][i] == m }
 *   w[f][g]       #{ i : valid(f, i) and g in obs(point_id[f][i]) }
 * Row f of the CSR holds the pairs (g, w[f][g]) with w > 0, strictly ascending in g; frames >= size get empty rows; row_ptr[max_frames] = E.  This is the
 * reference's loop (per mappoint of the frame, one increment per observer), so: w[f][f] = the valid rows of f (the self entry is kept); a frame without
 * a valid row has an EMPTY row, without a self entry; a point at two rows of f counts twice from f's side while f is ONE observer of it, so
 * w[f][g] = 2 with w[g][f] = 1 — the table is not symmetric.  STATED DIFFERENCE: the observer lists are those the id table implies; the reference reads
 * Mappoint::_obversers, which agrees with the frames' _mappoints in a map that passes CheckMap.
 * Rows >= n[f] and frames >= size are never read as ids and may hold anything.  An id outside [0, max_points) other than -1 never indexes memory: it is
 * counted in info[3] and treated as -1.
 *   _dev    asynchronous on `stream`, no host synchronisation, no allocation.  REPLACES the whole graph (a grouping or stored query queued on ANOTHER
 *           stream must have completed).  d_info i32 [4] (device): status (0 ok, 1 overflow), entries needed, valid (frame, row) entries, ids ignored as
 *           out of range.  More entries needed than max_edges: the graph becomes EMPTY (every row_ptr 0) and status is 1.
 *   host    the same on the context's stream, then a synchronisation; *n_edges = the entries needed; overflow is an error return (the graph is empty).
 * Return codes: no id table; more than 4096 frames in the database.  Three statements that agree byte for byte: covis_build_host
 * (airslam_amd/csrc/covis_core.h), the kernels (kernels_covis.hip) and tests/covis_ref.py.  Two builds of one table give the same bytes: the kernels'
 * integer atomics only add to counters whose final value is read.  OUT OF SCOPE: UpdateFrameCovisibility for a single frame (a CSR row cannot be
 * replaced in place). */
int airfe_bowdb_attach_point_ids(airfe_bowdb* db, int max_points);
int airfe_bowdb_set_point_ids_dev(airfe_bowdb* db, int first_frame, int B, const int32_t* d_ids, void* stream);   /* d_ids [B][cap] */
int airfe_bowdb_set_point_ids(airfe_bowdb* db, int first_frame, int B, const int32_t* ids);                   /* host buffer [B][cap] */
int airfe_bowdb_get_point_ids(airfe_bowdb* db, int first_frame, int B, int32_t* ids);                         /* host buffer [B][cap] */
int airfe_bowdb_build_covisibility_dev(airfe_bowdb* db, int32_t* d_info, void* stream);
int airfe_bowdb_build_covisibility(airfe_bowdb* db, int* n_edges);

/* ---- Map-point triangulation: Map::TriangulateMappoint (src/map.cc:367-414) for every point of a loaded map, on the device ---------------------------
 * The positions the point table holds, from what the database already stores: the frames' feature rows (x, y at columns 1 and 2), their poses
 * (airfe_bowdb_set_poses) and the map-point id of every row (the id table above).  The reference calls the function for an UnTriangulated point with
 * more than two observers at keyframe insertion (map.cc:64-66), from loop closure (map_refiner.cc:430) and from MergeMappointGroup (:702-704).
 * airfe_bowdb_attach_triangulation (needs airfe_bowdb_attach_point_ids; a second attach is a return code) allocates 8 bytes per feature row for the
 * observation segments and 32 bytes per point for the host form's outputs; nothing is allocated afterwards.  The marks and segment starts are the
 * covisibility build's work arrays: a covisibility build, a grouping or a stored query queued on ANOTHER stream must have completed.
 * THE STATEMENT (airslam_amd/csrc/triangulate_core.h; valid(f, i), size and n[f] as in the covisibility build):
 *   observers   the observation of point m in frame f is the FIRST row i of f with valid(f, i) and point_id[f][i] == m.  STATED DIFFERENCE: the reference
 *               keeps the last AddObverser per frame.  Observers are taken in ascending frame index (the reference's std::map order); nobs[m] = their number.
 *   per observer, with fxi = 1.0 / fx, fyi = 1.0 / fy (Camera::BackProjectMono, camera.cc:268-273) and R, c the rotation and translation of the stored Twc:
 *               b = (((double)x - cx) * fxi, ((double)y - cy) * fyi, 1);  v_r = (R[r][0] b0 + R[r][1] b1) + R[r][2] b2;  s = (v0 v0 + v1 v1) + v2 v2;
 *               w_r = v_r * (1.0 / s);  d = (v0 c0 + v1 c1) + v2 c2;  in observer order M[r][q] += w_r v_q, g_r += w_r d, C_r += c_r.
 *   system      A = n I - M, rhs = C - g (map.cc:398-403); a column-pivoted Householder QR of A by the rules of Eigen's ColPivHouseholderQR as far as they
 *               decide anything (pivot = the remaining column of largest squared norm, the first wins a tie; Eigen's reflector and its application);
 *               rank = #{ |R_kk| > 1e-5 max |R_kk| } (map.cc:405-409); with rank 3, x = P R^-1 Q^T rhs.  STATED DIFFERENCES: the remaining column norms
 *               are recomputed at every step instead of down-dated; byte equality with Eigen is NOT claimed (triangulate_core.h says what is).
 *   status      -1 no observer; 0 ok; 1 nobs < max(min_observers, 2); 2 rank < 3; 3 a non-finite keypoint, pose entry (rows 0 .. 2), s, system entry or
 *               result, or s == 0, among the point's observers.  xyz = NaN unless status is 0.  A bad point never changes another point's bytes.
 * Doubles, every sum sequential in the order written, no fused multiply-adds.  Three statements that agree byte for byte: triangulate_build_host
 * (triangulate_core.h), the kernels (kernels_triangulate.hip) and tests/triangulate_ref.py.  Each point's observations are SORTED by frame before they are
 * summed: no output byte depends on the order in which an atomic landed, and two calls give the same bytes.
 *   _triangulate_points_dev   cam: HOST f64 [4] = fx, fy, cx, cy.  d_xyz f64 [max_points][3], d_status / d_nobs i32 [max_points], d_info i32 [4] = points ok,
 *               points observed (status != -1), points of status 2, of status 3: every entry is written.  Asynchronous on `stream`, no host
 *               synchronisation, no allocation.  The point table is not touched.
 *   _triangulate_points       the same into host buffers on the context's stream, then a synchronisation; *n_ok = the points of status 0.
 *   _fill_points_dev          for every valid row (f, i) with id m and d_status[m] == 0: points[f][i] = d_xyz[m] (a point at two rows of a frame fills both);
 *               with only_missing only where the stored x is NaN (the reference's "only UnTriangulated points" rule).  Rows >= n[f], frames >= size and
 *               rows of points with status != 0 are not touched.  d_written i32 [1] = the rows written.  Asynchronous on `stream`; a relocalisation or loop
 *               detection reading the point table on ANOTHER stream must have completed.
 *   airfe_triangulate_point   the host core for one point without a context: Twc [n][16], xy f32 [n][2] in observer order, min_observers = 2;
 *               *status as above, xyz [3].
 * Return codes (nothing is changed then): no triangulation attached; more than 4096 frames in the database; fx or fy zero or non-finite; a NULL argument. */
int airfe_bowdb_attach_triangulation(airfe_bowdb* db);
int airfe_bowdb_triangulate_points_dev(airfe_bowdb* db, const double* cam, int min_observers, double* d_xyz, int32_t* d_status, int32_t* d_nobs,
                                       int32_t* d_info, void* stream);
int airfe_bowdb_triangulate_points(airfe_bowdb* db, const double* cam, int min_observers, double* xyz, int32_t* status, int32_t* nobs, int* n_ok);
int airfe_bowdb_fill_points_dev(airfe_bowdb* db, const double* d_xyz, const int32_t* d_status, int only_missing, int32_t* d_written, void* stream);
int airfe_triangulate_point(const double* cam, const double* Twc, const float* xy, int n, double* xyz, int* status);

/* ---- Map-point merge: the tail of MapRefiner::RelativatePoseEstimation (src/map_refiner.cc:338-372, :409-459) and MapRefiner::MergeMappoints /
 * MergeMappointGroup (:603-713), on the device ------------------------------------------------------------------------------------------------------
 * What turns a detected loop into a changed map: from airfe_loop_detect_batch_dev's outputs and the id and point tables to MERGED tables, on one stream,
 * nothing copied to the host, nothing allocated.  Afterwards airfe_bowdb_triangulate_points_dev + _fill_points_dev(only_missing) and
 * airfe_bowdb_build_covisibility_dev bring positions and graph in line (api.BowDatabase.loop_close_dev queues all of it).
 * airfe_bowdb_attach_merge (needs airfe_bowdb_attach_point_ids; a second attach is a return code) allocates 24 bytes per point (parent, flags, src, best,
 * root, the host form's map) and 4 bytes per feature row (the adoption staging); every call initialises the per-point arrays, so its cost grows with
 * max_points like the covisibility build's.
 * THE STATEMENT (airslam_amd/csrc/merge_core.h; valid(f, i), size, n[f] and max_points as in the covisibility build; an id is VALID iff it is in
 * [0, max_points); the point table is xyz[f][i]).  An id m is TRIANGULATED iff some valid row holding m has a non-NaN x; src(m) = the smallest key
 * f * cap + i of such a row.  Every gate reads the id table and the point table AS THEY WERE BEFORE THE CALL.
 *   (1) live entries.  For query q with d_stage[q] == 0, fq = d_qframe[q], b_f = d_loop[q] and list entry e < min(d_nmatch[q], mcap), (qi, ci) = d_idx[q][e]:
 *       dead if fq or b_f is outside 0 .. size - 1, if qi >= n[fq] or ci >= n[b_f] or either is negative, or if B = point_id[b_f][ci] is not valid.
 *       xyz[b_f][ci].x not NaN: live iff d_mask[q][e] != 0.  STATED DIFFERENCE: an outlier is dropped where the reference searches the inverted file
 *       (find_more_matches_in_group).  xyz[b_f][ci].x NaN: live iff the epipolar test of :338-352 passes on p1 = feat[fq][qi].xy, p2 = feat[b_f][ci].xy, in
 *       double, no fused multiply-adds, every 3 x 3 product element (a0 b0 + a1 b1) + a2 b2:  fxi = 1.0 / fx, fyi = 1.0 / fy,
 *       Kit = [fxi 0 0; 0 fyi 0; -(cx fxi) -(cy fyi) 1] (K^-T in closed form), tx = [tlq]x, F = ((Kit tx) Rlq) K;  el_r = (F[r][0] x1 + F[r][1] y1) + F[r][2];
 *       s = sqrt(el_0 el_0 + el_1 el_1);  er = ((x2 el_0 + y2 el_1) + el_2) / s;  passes iff er < 10 (the reference's signed comparison; a NaN er fails).
 *       STATED DIFFERENCES: the loop frame's keypoint is row ci, not GetKeypointIdx; every feature row counts as having a word.
 *   (2) adoption (:452-457).  A live entry whose point_id[fq][qi] is not valid: the row adopts B.  Several live entries adopting one row: the row takes the
 *       SMALLEST such B and all those B are joined into one group.  The row's xyz = xyz[src(B)] if B is triangulated, else NaN.  STATED DIFFERENCE: the
 *       reference inserts the point at the frame without AddObverser; here the id table IS the observer list.
 *   (3) pairs.  A live entry whose A = point_id[fq][qi] is valid gives the pair (A, B).
 *   (4) groups (:608-651) = the connected components over ids of the pairs and of (2)'s joins.  A group of one is untouched.
 *   (5) best (:674-681) = the group's smallest triangulated id; if none is triangulated, its smallest id.
 *   (6) relabel (:683-712), on the table.  Group G, best b, frame f, R = the valid rows of f whose id after adoption is in G.  Some row of R holds b: the rows
 *       holding b stay, every other row of R becomes id -1 with NaN xyz (its map point was erased; the reference leaves a bad pointer there).  Otherwise,
 *       with m* the smallest id in R and i* the first row of f holding m*: row i* gets id b and xyz[src(b)] (NaN if b is not triangulated), every other row
 *       of R becomes -1 / NaN.  Not touched: rows >= n[f], frames >= size, rows of ids in no group.
 *   (7) outputs, every entry written.  d_map i32 [max_points]: b for a member of a group, else the id itself.  d_info i32 [8]: live entries, entries dropped
 *       as outliers, entries dropped by the epipolar test, rows adopted (whatever (6) then makes of them), groups, ids removed (the sum of the group sizes
 *       minus the groups), rows relabelled to a best, rows cleared.
 * No output byte depends on the order of the queries or of a list's entries, or on the order in which an atomic landed (the kernels' atomics decide minima,
 * flag bits, counts and a union-find forest of which only each id's root, the smallest id of its component, is read); two calls on the same tables give the
 * same bytes.  Three statements that agree byte for byte: merge_build_host / merge_pairs_host (merge_core.h), the kernels (kernels_merge.hip) and
 * tests/merge_ref.py (whose epipolar gate is numpy's inv(K^T) tx R K: a decision, equal wherever er is not within rounding of 10).
 *   _merge_points_dev       steps (4) - (7) on an explicit pair list d_pairs i32 [P][2], the reference's merged_mappoints.  A pair with an id that is not valid
 *                           is ignored and counted: d_info = pairs taken, pairs ignored, 0, 0, then as above.  d_pairs may be NULL when P is 0.
 *   _merge_points           the same from host buffers (map [max_points], info [8]) on the context's stream, then a synchronisation.
 *   _loop_merge_batch_dev   steps (1) - (7) straight from the buffers airfe_loop_detect_batch_dev wrote (cam: HOST f64 [4] = fx, fy, cx, cy; d_mask u8
 *                           [Q][mcap], d_idx i32 [Q][mcap][2]); the per-query arrays may be NULL when Q is 0.
 * The _dev forms are asynchronous on `stream`, without host synchronisation or allocation; they CHANGE the id table and the point table in place: a
 * covisibility build, triangulation, relocalisation or loop detection on ANOTHER stream must have completed.
 * Return codes (nothing is changed then): no merge attached; more than 4096 frames in the database; Q > 4096; mcap > 1024; a NULL argument; fx or fy zero
 * or non-finite.
 * OUT OF SCOPE: find_more_matches_in_group and the inverted file; MergeMaplines; the pose graph; GlobalBA; track ids (SetTrackId). */
int airfe_bowdb_attach_merge(airfe_bowdb* db);
int airfe_bowdb_merge_points_dev(airfe_bowdb* db, const int32_t* d_pairs, int P, int32_t* d_map, int32_t* d_info, void* stream);
int airfe_bowdb_merge_points(airfe_bowdb* db, const int32_t* pairs, int P, int32_t* map, int32_t* info);
int airfe_bowdb_loop_merge_batch_dev(airfe_bowdb* db, const double* cam, const int32_t* d_qframe, int Q, const int* d_stage, const int32_t* d_loop,
                                     const double* d_Rlq, const double* d_tlq, const uint8_t* d_mask, const int32_t* d_idx, int mcap, const int* d_nmatch,
                                     int32_t* d_map, int32_t* d_info, void* stream);

/* ---- Junction term: junction_frame_scores * (1 + rate) of MapUser::Relocalization (src/map_user.cc:285-331), on the device ---------------------------
 * The number per stored frame that airfe_bowdb_group_dev / airfe_relocalize_batch_dev add to a group's score through d_extra [Q][N].  d_extra[q][deputy] is
 * all the grouping reads, so the term is computed for every stored frame rather than for the group frames: the grouping is the same.
 * WHERE THE JUNCTION DATABASE LIVES.  The reference's junction database has a vocabulary of its own (map_refiner.cc:956-999: k = 10, L = 3, TF-IDF, L1).
 * Here: a second airfe_ctx with that vocabulary loaded (airfe_bow_load; a context needs no network pack) and on it a second airfe_bowdb, `jdb`
 * (keep_features = 0 is enough).  Frame f of jdb IS frame f of the point database: same insertion order, the caller's responsibility.  At most 1024
 * junctions per frame (the BoW kernels' limit).  Training the vocabulary (jun_voc->create) stays the caller's.
 * RESTATED (junction_core.h: one statement the kernels and the host core both call; tests/junction_ref.py restates the reference literally):
 *   connections   Frame::FindJunctionConnections (src/frame.cc:581-629).  Junction row i = (score, jx, jy, ...) sits at pixel
 *                 ((int)((double)jx + 0.5), (int)((double)jy + 0.5)); of several junctions in one pixel the HIGHEST index owns it (:587-591 overwrites in
 *                 index order).  An endpoint (ex, ey) has xi = int(ex + 0.5), yi = int(ey + 0.5) and matches the junction that owns the cell with the
 *                 smallest key (|yi - r| + |xi - c|, r, c) over r in [max(yi - 2, 0), min(yi + 2, H - 1)], c in [max(xi - 2, 0), min(xi + 2, W - 1)]
 *                 — the row-major scan of :600-614 with its strict < and its early return at distance 0 — or nothing (-1).  A line with both ends
 *                 matched to a and b gives the directed edges (a, b) and (b, a) (a == b: the self loop (a, a), an edge like any other, :626-627); the
 *                 second end is not looked at without the first (:621).  Output: the DISTINCT directed edges ascending by (a, b), i32 [ecap][2], their
 *                 count, and optionally per line the pair (a, b) or (-1, -1).  The device keeps the junctions' pixels in LDS and every endpoint
 *                 scans them: no H x W map.
 *   tables        from word [nj] (u32, UINT_MAX = a word of weight 0: database.cc:70-75) and the edges.  WORD TABLE: the distinct valid words ascending,
 *                 each with cnt = the junctions holding it (the inverted file's list, database.cc:98-106) and conn = those of them with at least one
 *                 edge.  KEY TABLE: the distinct word[a] << 32 | word[b] over the edges whose two words are valid, ascending, each with its multiplicity.
 *   term          :293-327 builds match_matrix[i][j] = (word_q[i] == word_f[j], the word valid) and counts over it.  With these tables
 *                 match_num = sum over words w of conn_q(w) * cnt_f(w)  (:313-315) and line_match_num = sum over keys k of n_q(k) * n_f(k)  (:316-325),
 *                 both i32 (ecap <= 4096 and 1024 junctions: <= 2^24 and <= 2^20).  rate = match_num > 0 ? (double)line_match_num / match_num : 0  (:329);
 *                 extra = score * (1.0 + rate)  (:330-331) with score = L1Scoring::score(v1 = the stored frame's junction vector, v2 = the query's) as the
 *                 unchanged query kernel computes it on jdb; one division, one add, one multiply, no fused multiply-add.  The counts are integer sums and
 *                 do not depend on their order.
 * THE QUIRK KEPT: invalid words never match each other (:300 skips them; they are in no inverted file).
 * STATED DIFFERENCES: a junction whose pixel lies outside [0, W) x [0, H) owns no cell, where the reference writes out of bounds; an endpoint whose
 * ex + 0.5 or ey + 0.5 is not finite or not inside (-2^31, 2^31) matches nothing, where the reference's conversion is undefined; more than ecap distinct
 * edges sets the frame's STATUS to 2 (0 = ok), gives it no edges and a term of 0.0 with counts 0 — never a shorter list.  (nj > 1024 cannot reach the
 * device entries: capJ > 1024 is a return code; the host core answers it with status 2.)
 *   airfe_junction_connections_batch_dev   B frames in place on the batched PLNet outputs: d_lines [B][capL][4] f64, d_nlines [B], d_junc [B][capJ][259],
 *       d_njunc [B]; counts are clamped to their capacities.  -> d_edge [B][ecap][2], d_nedge [B], d_status [B], d_line_pair [B][capL][2] or NULL (rows
 *       below the frame's line count).  One workgroup per frame, sort and deduplication in LDS; a frame's bytes depend on neither B nor its position;
 *       nothing is allocated; rows past the counts are neither read as data nor written.
 *   airfe_junction_connections             the host core, one frame, no device work.  Returns 2 (and *nedge = 0) for status 2.
 *   airfe_bowdb_attach_junctions(jdb, ecap, max_queries)   allocates, once: per stored frame its words [max_frames][cap], their count, the two tables and a
 *       status (1 = no junction state yet: such a frame's term is 0.0); the same tables, the dense score and the composites' chain for max_queries
 *       frames.  Nothing is allocated afterwards.  A second attach is a return code.
 *   airfe_bowdb_set_junctions_dev / _set_junctions   store the words of frames first_frame .. first_frame + B - 1 and build their tables: d_word [B][cap]
 *       (cap = the database's), d_nj [B], d_edge [B][ecap][2] (ecap = the attached one), d_nedge [B], d_status [B] or NULL (a non-zero entry: status 2).
 *       An edge with an index outside [0, nj) is ignored.  The host form takes at most max_queries frames per call and synchronises.
 *   airfe_bowdb_get_junctions              reads back (host buffers, any may be NULL): word [B][cap], nj [B], uword / wcnt / wconn [B][cap], nuw [B],
 *       ukey u64 / kcnt [B][ecap], nuk [B], status [B].  Entries past nuw / nuk are whatever they were.
 *   airfe_bowdb_junction_term_batch_dev    Q queries: d_ids / d_vals [Q][cap], d_nw [Q] and d_word [Q][cap] = airfe_bow_vector_batch_dev's outputs for the
 *       query frames' junction rows on jdb's context; d_nj [Q]; d_edge [Q][ecap][2], d_nedge, d_qstatus [Q] (or NULL) = the connections' outputs.
 *       -> d_extra f64 [Q][N], d_match_num / d_line_match_num i32 [Q][N] or NULL, N = jdb's size: EVERY one of the Q N entries is written.  A query or a
 *       stored frame with a non-zero status gets extra = 0.0 and counts 0.  Grid: (query, slice of frames) as the query kernel's; the query's tables
 *       in LDS; a wave per stored frame, integer partial sums reduced across the wave.
 *   airfe_bowdb_junction_extra_batch_dev   the composite, from the query frames' raw junction rows and lines to d_extra on one stream:
 *       airfe_bow_vector_batch_dev's code, the connections, the tables, the query, the term — byte for byte those steps done one at a time.  capJ must be
 *       jdb's cap.  The caller passes d_extra to airfe_relocalize_batch_dev on the same stream.
 *   airfe_bowdb_add_junction_frames_batch_dev   the same chain for B map frames: vector, add to jdb, connections, set_junctions — BuildJunctionDatabase's
 *       second loop plus FindJunctionConnections (map_refiner.cc:977, 986-994).  B <= max_queries per call.
 * Return codes that change nothing: capJ > 1024, ecap > 4096, Q (or B) > max_queries, a database without attach_junctions, frames beyond max_frames. */
int airfe_junction_connections_batch_dev(airfe_ctx* ctx, const double* d_lines, const int* d_nlines, int capL, const float* d_junc, const int* d_njunc,
                                         int capJ, int B, int W, int H, int32_t* d_edge, int ecap, int* d_nedge, int* d_status, int32_t* d_line_pair,
                                         void* stream);
int airfe_junction_connections(airfe_ctx* ctx, const double* lines, int nl, const float* junc, int nj, int W, int H, int32_t* edge, int ecap, int* nedge,
                               int32_t* line_pair);
int airfe_bowdb_attach_junctions(airfe_bowdb* jdb, int ecap, int max_queries);
int airfe_bowdb_set_junctions_dev(airfe_bowdb* jdb, int first_frame, int B, const uint32_t* d_word, const int* d_nj, const int32_t* d_edge,
                                  const int* d_nedge, const int* d_status, void* stream);
int airfe_bowdb_set_junctions(airfe_bowdb* jdb, int first_frame, int B, const uint32_t* word, const int* nj, const int32_t* edge, const int* nedge,
                              const int* status);
int airfe_bowdb_get_junctions(airfe_bowdb* jdb, int first_frame, int B, uint32_t* word, int* nj, uint32_t* uword, int32_t* wcnt, int32_t* wconn, int* nuw,
                              uint64_t* ukey, int32_t* kcnt, int* nuk, int* status);
int airfe_bowdb_junction_term_batch_dev(airfe_bowdb* jdb, const uint32_t* d_ids, const double* d_vals, const int* d_nw, const uint32_t* d_word,
                                        const int* d_nj, const int32_t* d_edge, const int* d_nedge, const int* d_qstatus, int Q, double* d_extra,
                                        int32_t* d_match_num, int32_t* d_line_match_num, void* stream);
int airfe_bowdb_junction_extra_batch_dev(airfe_bowdb* jdb, const float* d_junc, const int* d_njunc, int capJ, const double* d_lines, const int* d_nlines,
                                         int capL, int Q, int W, int H, double* d_extra, int32_t* d_match_num, int32_t* d_line_match_num, void* stream);
int airfe_bowdb_add_junction_frames_batch_dev(airfe_bowdb* jdb, const float* d_junc, const int* d_njunc, int capJ, const double* d_lines,
                                              const int* d_nlines, int capL, int B, int W, int H, void* stream);

/* ---- the step BEFORE the path: rectification ------------------------------------------------------- */
/* ≙ the maps Camera's constructor builds with cv::initUndistortRectifyMap (src/camera.cc:60-75; _mapl1/_mapl2 = side 0, _mapr1/_mapr2 =
 *   side 1): CV_32FC1 x / y maps [h][w], uploaded once.  The map CONSTRUCTION (stereoRectify etc.) stays reference code. */
int airfe_set_rectify_maps(airfe_ctx* ctx, int side, const float* mapx, const float* mapy, int h, int w);
/* ≙ Camera::UndistortImage (src/camera.cc:161-182: cv::remap(..., INTER_LINEAR), BORDER_CONSTANT 0) + FeatureDetector::Detect on its
 *   result, in one call: raw HOST image in; rect_out (HOST, h x w tight rows, may be NULL) receives the rectified image the tracker and
 *   the visualisation still need (map_builder.cc:43,71-72,177); feat / n as airfe_detect_points (feat may be NULL: rectify only).
 *   The rectified image goes from the remap kernel straight into the detector's pre-process without leaving the device. */
int airfe_rectify_detect_points(airfe_ctx* ctx, int side, const uint8_t* raw, int h, int w, int stride, uint8_t* rect_out, float* feat,
                                int cap, int* n);
/* device-resident batch form: d_raw / d_rect [B] images (image b at + b * img_stride, rows stride bytes apart) */
int airfe_rectify_batch_dev(airfe_ctx* ctx, int side, const uint8_t* d_raw, int B, int h, int w, int stride, size_t img_stride,
                            uint8_t* d_rect, int rstride, size_t rimg_stride, void* stream);

/* ---- device-resident batch pipeline (NEW: no reference counterpart) ------------------------------------ */
/* d_gray: [B] images, image b at d_gray + b*img_stride, rows `stride` bytes apart.  d_feat [B][cap][259], d_n [B]. */
int airfe_detect_points_batch_dev(airfe_ctx* ctx, const uint8_t* d_gray, int B, int h, int w, int stride,
                                  size_t img_stride, float* d_feat, int cap, int* d_n, void* stream);
/* LightGlue on B pairs of device feature matrices (259-float rows, ORIGINAL pixel coords; NormalizeKeypoints with
 *   cfg.image_width/height is applied on the device exactly as src/point_matcher.cc:39-48 does on the host).
 *   d_idx [B][mcap][2], d_score [B][mcap], d_nmatch [B].
 *   Empty frames: d_n0[b] = 0 and / or d_n1[b] = 0 is valid input (a frame without detections; the counts are read on the device, there is no host-side
 *   early-out).  Such a pair gets d_nmatch[b] = 0 and none of its d_idx / d_score entries is written, in either assignment form
 *   (≙ src/point_matcher.cc:53-55, which returns before the engine runs); the other pairs of the batch are not affected. */
int airfe_match_lightglue_batch_dev(airfe_ctx* ctx, const float* d_f0, const int* d_n0, const float* d_f1, const int* d_n1,
                                    int B, int cap, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, void* stream);
/* SuperGlue on B pairs (as above; NormalizeKeypoints scale 0.7, src/point_matcher.cc:58): d_idx0 / d_idx1 [B][cap] (-1 = unmatched,
 *   decode semantics of src/super_glue.cpp:339-367), d_ms0 / d_ms1 [B][cap] floats. */
int airfe_match_superglue_batch_dev(airfe_ctx* ctx, const float* d_f0, const int* d_n0, const float* d_f1, const int* d_n1, int B, int cap,
                                    int32_t* d_idx0, int32_t* d_idx1, float* d_ms0, float* d_ms1, void* stream);
/* One "stereo detect+match pair" x B (≙ map_builder.cc:85-86: Detect(L,R) + MatchingPoints(L,R)). */
int airfe_stereo_batch_dev(airfe_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int B, int h, int w, int stride,
                           size_t img_stride, float* d_featL, float* d_featR, int cap, int* d_nL, int* d_nR,
                           int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, void* stream);
/* NEW (no reference counterpart: PLNet::infer, src/plnet.cpp:221-244, is one image per call): PLNet over B device-resident images in one
 * pass — points exactly as airfe_detect_points_batch_dev; the line branch (stage-0 line head, wireframe_matcher, stage 1, line filter)
 * for every image; junction_detector (+ descriptors) for the FIRST `junction_images` images.  Per image the results are the bits
 * airfe_detect_plnet returns for it.
 *   d_lines [B][capL][4] doubles (x1,y1,x2,y2 in original-image pixels), d_nlines [B] (<= capL)
 *   d_junc [junction_images][capJ][259], d_njunc [junction_images] (<= capJ)
 *   d_found (may be NULL) [B + junction_images]: lines that passed the filter per image, then junctions found per image — a value
 *   above capL / capJ is an overflow the caller must treat as an error (the reference has no limits; the batch-1 entry reports it itself) */
int airfe_detect_plnet_batch_dev(airfe_ctx* ctx, const uint8_t* d_gray, int B, int h, int w, int stride, size_t img_stride, float* d_feat,
                                 int cap, int* d_n, double* d_lines, int capL, int* d_nlines, float* d_junc, int capJ, int* d_njunc,
                                 int junction_images, int* d_found, void* stream);
/* One "stereo detect+match pair" x B with the PLNet detector (≙ map_builder.cc:85-86 with use_superpoint = 0: Detect(L, R, lines, junctions)
 * + MatchingPoints): one detector pass over the 2 B images, lines of all of them (d_lines [2B][capL][4], d_nlines [2B]: left images first),
 * junctions of the left ones only (feature_detector.cc:100-101), LightGlue on the points.  d_found (may be NULL) [3B]. */
int airfe_stereo_plnet_batch_dev(airfe_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int B, int h, int w, int stride,
                                 size_t img_stride, float* d_featL, float* d_featR, int cap, int* d_nL, int* d_nR, double* d_lines,
                                 int capL, int* d_nlines, float* d_juncL, int capJ, int* d_njuncL, int* d_found, int32_t* d_idx,
                                 float* d_score, int mcap, int* d_nmatch, void* stream);
/* NEW (no reference counterpart as a batch; the per-frame functions are AssignPointsToLines / MatchLines, src/line_processor.cc:68-180, called
 * right behind Detect / MatchingPoints at src/frame.cc:125,177,184): the same two functions over B device-resident frames, reading the outputs of
 * airfe_detect_plnet_batch_dev / airfe_stereo_plnet_batch_dev / airfe_match_lightglue_batch_dev IN PLACE.  Per frame the results are the bits
 * airfe_assign_points_to_lines / airfe_match_lines return for it.
 *   relation as CSR per frame: d_row_ptr [B][capL + 1], d_pt_idx [B][capE], d_pt_dist [B][capE] doubles (ascending point index per line, like the
 *   reference's std::map<int, double>); d_total (may be NULL) [B] = entries found: a value above capE is an overflow (entries beyond capE are dropped) */
int airfe_assign_points_to_lines_batch_dev(airfe_ctx* ctx, const double* d_lines, const int* d_nlines, int capL, const float* d_feat, const int* d_n,
                                           int cap, int B, int32_t* d_row_ptr, int32_t* d_pt_idx, double* d_pt_dist, int capE, int* d_total,
                                           void* stream);
/*   d_matches [B][mcap][2] + d_nmatch [B]: the matcher's (idx0, idx1) lists; filter3 (HOST, may be NULL) = {min_x_diff, max_x_diff, max_y_diff}: the
 *   disparity band Frame::AddRightFeatures applies to the stereo matches before MatchLines (src/frame.cc:147-160), evaluated on d_feat0 / d_feat1
 *   [B][cap][259]; d_line_matches [B][capL]: index of the matched line of frame 1 or -1, for the first d_nlines0[b] lines of every frame */
int airfe_match_lines_batch_dev(airfe_ctx* ctx, const int32_t* d_row_ptr0, const int32_t* d_pt_idx0, const int* d_nlines0, const int* d_n0,
                                const int32_t* d_row_ptr1, const int32_t* d_pt_idx1, const int* d_nlines1, const int* d_n1, int capL, int capE,
                                const int32_t* d_matches, const int* d_nmatch, int mcap, int B, const double* filter3, const float* d_feat0,
                                const float* d_feat1, int cap, int32_t* d_line_matches, void* stream);
/* NEW (no reference counterpart: the reference copies whole bindings back inside every infer(), src/plnet.cpp:237, buffers.h:237-417): the VALID rows of device
 * result buffers to wherever a kernel can write — device memory or host-mapped pinned memory (hipHostMalloc) — in ONE launch on `stream`.  Job j copies
 * min(*cnt[j], cap[j]) rows (cnt[j] == NULL: cap[j] rows) of row_bytes[j] bytes (a multiple of 4) from src[j] to dst[j]; the counts are read on the device, so the
 * caller needs no synchronisation to learn them first, and only the rows that exist cross PCIe (a batch entry's junction buffer is 1 MB per image at its capacity for
 * ~150 rows of 1 KB).  The five arrays are HOST arrays of njobs entries, read before the call returns.  Asynchronous: the copies are complete when `stream` is. */
int airfe_copy_rows_dev(airfe_ctx* ctx, int njobs, const void* const* src, void* const* dst, const int* const* cnt, const uint32_t* row_bytes,
                        const uint32_t* cap, void* stream);
/* The same, packed: job j's valid rows go to d_packed + d_offsets[j] (16-byte aligned, jobs back to back in order), d_offsets[njobs] = the bytes used; the
 * offsets are an exclusive scan of the counts taken ON THE DEVICE (two launches on `stream`).  d_packed (device) must hold the sum of the jobs' capacities rounded
 * up to 16 bytes each; d_offsets (device) njobs + 1 entries.  For a consumer that wants the results of a large batch on the host through the copy ENGINES: read
 * d_offsets (a few KB), then copy d_packed[0 .. d_offsets[njobs]) with hipMemcpyAsync — no kernel sits on the stream's hardware queue while the bytes cross PCIe
 * (bench.py --io host: one kernel writing the rows into pinned memory itself reaches the same 55 GB/s but runs in line with the next step's kernels wherever the
 * two streams share a hardware queue). */
int airfe_pack_rows_dev(airfe_ctx* ctx, int njobs, const void* const* src, const int* const* cnt, const uint32_t* row_bytes, const uint32_t* cap, void* d_packed,
                        unsigned long long* d_offsets, void* stream);
/* synchronises the context's own stream; also reports (once) a Sinkhorn rendezvous time-out of an earlier SuperGlue call */
int airfe_sync(airfe_ctx* ctx);
/* SuperGlue's error channel for callers of the asynchronous *_dev entries who synchronise their OWN stream: synchronises `stream` (the one the
 * call was issued on; NULL = the context's), then reads and clears the Sinkhorn time-out flag.  0 = the scores of every call so far are valid;
 * 1 = a cooperative rendezvous timed out in one of them (its outputs are NaN / -1), airfe_last_error says so.  The reference has no counterpart:
 * its engine call is synchronous and cannot fail this way (src/super_glue.cpp:185-189). */
int airfe_superglue_status(airfe_ctx* ctx, void* stream);

/* ---- per-stage hipEvent timers (measurement; SURVEY.md §5 "tracing") ----------------------------------- */
/* select + reset: on = 0 off, on < 0 every stage, on > 0 bit mask (bit i = stage i).  A selected stage has each of its
   kernel groups bracketed by two events on the launch stream; an event pair costs ~4 us of stream time (measured: all
   stages on = +8 % per step), so timed runs select only the stage they need. */
int airfe_profile_enable(airfe_ctx* ctx, int on);
int airfe_profile_stages(void);
const char* airfe_profile_stage_name(int i);
/* synchronises, then sums per stage: elapsed ms, algorithmic FLOPs, algorithmic bytes, launch groups; resets */
int airfe_profile_read(airfe_ctx* ctx, double* ms, double* flops, double* bytes, int* launches);

/* The inspection hooks the parity tests use (airfe_debug_*) are NOT part of the product boundary: include/airfe_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* AIRFE_H_ */
