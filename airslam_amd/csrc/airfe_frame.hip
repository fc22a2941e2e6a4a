// airfe — the frame entries of libairfe.so (include/airfe.h): detection, PLNet and stereo over host and device images, the stereo keyframe and the
// track / promote / adopt entries of the batch-1 regime.  The pieces their queues and read-backs share are stated once, in front of the entries.
#include "airfe_host.h"

int upload_reference(airfe_ctx* c, DrainOnError& drain, size_t off, const float* ref_feat, int n_ref, hipStream_t st) {
  *reinterpret_cast<int*>(c->pin + off) = n_ref;
  if (n_ref > 0) memcpy(c->pin + off + 64, ref_feat, (size_t)n_ref * AIRFE_FEAT_DIM * 4);
  drain.ref_uploaded = true;       // (the reference count becomes valid with the queued upload; an error below takes it back)
  HIPCHK(c, hipMemcpyAsync(c->ref_blk.p, c->pin + off, 64 + (size_t)n_ref * AIRFE_FEAT_DIM * 4, hipMemcpyHostToDevice, st));
  c->ref_n = n_ref;
  return 0;
}

int rows_home(airfe_ctx* c, const DevBlock& blk, size_t bytes, hipStream_t s2) {
  HIPCHK(c, hipMemcpyAsync(c->pin, blk.p, bytes, hipMemcpyDeviceToHost, s2));
  HIPCHK(c, hipEventRecord(c->ev_feat, s2));
  return 0;
}

int rows_second_trip(airfe_ctx* c, std::initializer_list<RowsPart> parts, hipStream_t st) {
  size_t total = 0, o = 0;
  for (const RowsPart& p : parts) total += p.bytes;
  if (!total) return 0;
  if (ensure_pin(c, total)) return 1;
  for (const RowsPart& p : parts) {
    if (p.bytes) HIPCHK(c, hipMemcpyAsync(c->pin + o, p.dev, p.bytes, hipMemcpyDeviceToHost, st));
    o += p.bytes;
  }
  HIPCHK(c, hipStreamSynchronize(st));
  o = 0;
  for (const RowsPart& p : parts) {
    if (p.bytes) memcpy(p.host, c->pin + o, p.bytes);
    o += p.bytes;
  }
  return 0;
}

int upload_stage0(airfe_ctx* c, const airfe_plnet_stage0* s0, hipStream_t st) {
  c->wf_counted = false;               // host tensors: nothing has counted their kept proposals
  const size_t NP = KEEP_CAP;
  float* d = c->s0_stage;
  HIPCHK(c, hipMemcpyAsync(d + SG_JUNCS, s0->juncs_pred, 600 * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d + SG_LP, s0->lines_pred, NP * 16, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d + SG_KEEP, s0->iskeep, NP * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d + SG_MIN, s0->idx_junc_to_end_min, NP * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d + SG_MAX, s0->idx_junc_to_end_max, NP * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->s0_loi, s0->loi_features, (size_t)128 * 128 * 128 * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d + SG_THIN, s0->loi_features_thin, (size_t)4 * 128 * 128 * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d + SG_AUX, s0->loi_features_aux, (size_t)4 * 128 * 128 * 4, hipMemcpyHostToDevice, st));
  return 0;
}

// ONE image through host buffers, detected and matched against rows that are already on the device, as one queue: the image goes up, the detector runs, the
// new rows come back on the side stream while LightGlue runs, then the counts and [idx | score].  What airfe_track_frame and airfe_promote_frame vary:
struct FrameMatch {
  const char* name;                    // the entry's, for the error texts
  const uint8_t* gray; int h, w, stride;
  DevBlock* out;                       // receives [counts {n, -, nmatch} | the image's rows | idx | score]
  DevBlock* first;                     // [count | rows] of the match's first side: ref_blk (the last keyframe's) or tk_blk (the last tracked frame's)
  const int* first_n;                  // ... and its count as the host knows it (ref_n / tk_n): decides "an empty side means no matches"
  const float* ref_feat; int n_ref;    // first == ref_blk: rows to upload there first (NULL: the rows kept from an earlier call)
  bool reject;                         // the context's outlier_rejection applies to the list (map_builder.cc:101 passes true, :107 false)
  bool sets_tk_n;                      // the image's rows are the ones airfe_promote_frame / airfe_adopt_reference work on afterwards
  float* feat; int* n; int32_t* match_idx; float* match_score; int* nmatch;
};
static int frame_match_host(airfe_ctx* c, const FrameMatch& f) {
  const int Np = c->cfg.max_keypoints;
  const bool ref = f.first == &c->ref_blk;
  hipStream_t st = c->stream;
  const size_t fb = (size_t)Np * AIRFE_FEAT_DIM * 4, early = 64 + fb, late = early + 64;
  // device block: [counts | new rows | idx | score]; the reference block [count | reference rows] is kept from call to call
  if (reserve(c, *f.out, 64 + fb + (size_t)Np * 12, c->stream)) return 1;
  if (ref && reserve(c, c->ref_blk, 64 + fb, c->stream)) return 1;
  int* cnt = f.out->at<int>(0);
  float* d_new = f.out->at<float>(64);
  int32_t* d_idx = f.out->at<int32_t>(64 + fb);
  float* d_sc = f.out->at<float>(64 + fb + (size_t)Np * 8);
  const int* d_nfirst = f.first->at<const int>(0);
  const float* d_first = f.first->at<const float>(64);
  // pinned block: the image, then (64-byte aligned) the reference on its way up; [counts | new rows], the final [counts] and [idx | score] on their way home
  const size_t ib = (size_t)(f.h - 1) * f.stride + f.w, ioff = (ib + 63) / 64 * 64;
  if (reserve(c, c->st_img, (size_t)f.h * f.stride, c->stream)) return 1;
  if (ensure_pin(c, std::max(ref ? ioff + 64 + fb : ib, late + (size_t)Np * 12))) return 1;
  if (ref && !f.ref_feat && c->ref_n < 0) return fail(c, std::string(f.name) + ": no reference features were ever given (ref_feat == NULL on the first call)");
  memcpy(c->pin, f.gray, ib);
  DrainOnError drain{c, true};
  HIPCHK(c, hipMemsetAsync(cnt, 0, 64, st));
  HIPCHK(c, hipMemcpyAsync(c->st_img.p, c->pin, ib, hipMemcpyHostToDevice, st));
  if (f.ref_feat && upload_reference(c, drain, ioff, f.ref_feat, f.n_ref, st)) return 1;
  if (detect_dev(c, c->st_img.p, 1, f.h, f.w, f.stride, (size_t)f.h * f.stride, d_new, Np, cnt, st)) return 1;
  HIPCHK(c, hipEventRecord(c->ev_fork, st));                         // the new rows go home on the side stream, beside the matcher
  HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
  if (rows_home(c, *f.out, early, c->stream2)) return 1;
  if (lightglue_dev(c, d_first, d_nfirst, d_new, cnt, 1, Np, AIRFE_FEAT_DIM, 1, 1, d_idx, d_sc, Np, cnt + 2, nullptr, st)) return 1;
  if (f.reject && c->outlier_rejection && fransac_queue(c, d_first, d_new, 1, Np, d_idx, d_sc, Np, cnt + 2, nullptr, st)) return 1;   // point_matcher.cc:95-104
  HIPCHK(c, hipMemcpyAsync(c->pin + early, cnt, 64, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(c->pin + late, d_idx, (size_t)Np * 12, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipEventSynchronize(c->ev_feat));
  const int nn = *f.n = rows_out(c, 0, f.feat);
  HIPCHK(c, hipStreamSynchronize(st));
  drain.armed = false;
  if (saturation_status(c)) { *f.n = 0; return 1; }
  if (f.sets_tk_n) c->tk_n = nn;
  if (nn < 1 || *f.first_n < 1) return 0;                            // point_matcher.cc:53-55
  const int nm = std::min(reinterpret_cast<const int*>(c->pin + early)[2], Np);
  matches_out(c, late, (size_t)Np * 8, 0, nm, f.match_idx, f.match_score);
  *f.nmatch = nm;
  return 0;
}

extern "C" {

int airfe_detect_points_batch_dev(airfe_ctx* c, const uint8_t* d_gray, int B, int h, int w, int stride, size_t img_stride,
                                  float* d_feat, int cap, int* d_n, void* stream) try {
  AIRFE_ENTER(c);
  return detect_dev(c, d_gray, B, h, w, stride, img_stride, d_feat, cap, d_n, stream_of(c, stream));
} AIRFE_CATCH(c)

int airfe_detect_points(airfe_ctx* c, const uint8_t* gray, int h, int w, int stride, float* feat, int cap, int* n) try {
  AIRFE_ENTER(c);
  if (cap < c->cfg.max_keypoints) return fail(c, "feature capacity < max_keypoints");
  if (upload_image(c, gray, h, w, stride)) return 1;
  if (detect_dev(c, c->st_img.p, 1, h, w, stride, (size_t)h * stride, c->st_feat0, c->Np, c->st_n0, c->stream)) return 1;
  // one D2H of [count | max_keypoints feature rows] into the pinned block (st_n0 and st_feat0 are one device block), rows copied out after the sync
  const size_t out_bytes = 64 + (size_t)c->cfg.max_keypoints * AIRFE_FEAT_DIM * 4;
  if (ensure_pin(c, out_bytes)) return 1;
  HIPCHK(c, hipMemcpyAsync(c->pin, c->io_in, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (saturation_status(c)) return 1;
  *n = rows_out(c, 0, feat);
  return 0;
} AIRFE_CATCH(c)

/* raw HOST image -> rectified image (HOST, tight rows, may be NULL) + point features of the RECTIFIED image: the rectified
   image never leaves the device on its way into the detector */
int airfe_rectify_detect_points(airfe_ctx* c, int side, const uint8_t* raw, int h, int w, int stride, uint8_t* rect_out, float* feat,
                                int cap, int* n) try {
  AIRFE_ENTER(c);
  if (feat && cap < c->cfg.max_keypoints) return fail(c, "feature capacity < max_keypoints");
  if (upload_image(c, raw, h, w, stride)) return 1;
  if (reserve(c, c->st_rect, (size_t)h * w, c->stream)) return 1;
  if (airfe_rectify_batch_dev(c, side, c->st_img.p, 1, h, w, stride, (size_t)h * stride, c->st_rect.p, w, (size_t)h * w, c->stream)) return 1;
  int nn = 0;
  if (feat) {
    if (detect_dev(c, c->st_rect.p, 1, h, w, w, (size_t)h * w, c->st_feat0, c->Np, c->st_n0, c->stream)) return 1;
    HIPCHK(c, hipMemcpyAsync(&nn, c->st_n0, 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (rect_out) HIPCHK(c, hipMemcpyAsync(rect_out, c->st_rect.p, (size_t)h * w, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (feat && saturation_status(c)) return 1;
  if (feat && nn > 0) HIPCHK(c, hipMemcpy(feat, c->st_feat0, (size_t)nn * AIRFE_FEAT_DIM * 4, hipMemcpyDeviceToHost));
  if (n) *n = nn;
  return 0;
} AIRFE_CATCH(c)

int airfe_stereo_batch_dev(airfe_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int B, int h, int w, int stride,
                           size_t img_stride, float* d_featL, float* d_featR, int cap, int* d_nL, int* d_nR, int32_t* d_idx,
                           float* d_score, int mcap, int* d_nmatch, void* stream) try {
  AIRFE_ENTER(c);
  hipStream_t st = stream_of(c, stream);
  if (c->prec != 2 && 2 * B <= c->Dmax) {        // left and right images as ONE detector batch
    if (detect_dev2(c, d_left, d_right, B, h, w, stride, img_stride, d_featL, d_featR, cap, d_nL, d_nR, st)) return 1;
  } else {
    if (detect_dev(c, d_left, B, h, w, stride, img_stride, d_featL, cap, d_nL, st)) return 1;
    if (detect_dev(c, d_right, B, h, w, stride, img_stride, d_featR, cap, d_nR, st)) return 1;
  }
  return lightglue_dev(c, d_featL, d_nL, d_featR, d_nR, B, cap, AIRFE_FEAT_DIM, 1, 1, d_idx, d_score, mcap, d_nmatch, nullptr, st);
} AIRFE_CATCH(c)

int airfe_detect_plnet(airfe_ctx* c, const uint8_t* gray, int h, int w, int stride, const airfe_plnet_stage0* s0, float* feat,
                       int cap, int* n, double* lines, int capL, int* nlines, float* junc, int capJ, int* njunc,
                       int want_junctions) try {
  AIRFE_ENTER(c);
  if (nlines) *nlines = 0;
  if (njunc) *njunc = 0;
  const bool lines_on = (s0 || c->has_s0);
  if (!lines_on) return airfe_detect_points(c, gray, h, w, stride, feat, cap, n);   // no line branch available: points only (the shim says so, loudly, at build())
  if (!c->has_s1) return fail(c, "PLNet stage-1 weights were not loaded (cfg.plnet_s1_pack)");
  if (cap < c->cfg.max_keypoints) return fail(c, "feature capacity < max_keypoints");
  // Everything is QUEUED before the first synchronisation (round 4; before: the point branch was synchronised and copied out first): image up,
  // point branch (plnet.cpp:560), line branch + tail, then [count | feature rows] and the three line / junction counts come back in one wait.
  hipStream_t st = c->stream;
  if (upload_image(c, gray, h, w, stride)) return 1;
  if (detect_dev(c, c->st_img.p, 1, h, w, stride, (size_t)h * stride, c->st_feat0, c->Np, c->st_n0, st)) return 1;
  if (s0) {
    if (upload_stage0(c, s0, st)) return 1;
  } else if (line_branch_dev(c, st, 0, 1, false)) {   // the stage-0 line branch on the device: nothing crosses PCIe (the reference moves
    return 1;                                         // 15.5 MB D2H + 9.7 MB H2D here, plnet.cpp:237,494-509)
  }
  int* nl_d = c->d_nlines;                            // [0] kept (<= LINE_CAP: the staging holds every candidate), [Lmax] found
  int *nj_d = c->d_njunc, *njf_d = c->d_njunc + c->Lmax;
  if (line_tail_dev(c, 0, 1, s0 != nullptr, h, w, c->d_lines, LINE_CAP, nl_d, nl_d + c->Lmax, c->junc_feat, JUNC_CAP, nj_d, njf_d,
                    want_junctions ? 1 : 0, st))
    return 1;
  const size_t fbytes = 64 + (size_t)c->cfg.max_keypoints * AIRFE_FEAT_DIM * 4;
  if (ensure_pin(c, fbytes + 64)) return 1;
  int* cnt = reinterpret_cast<int*>(c->pin + fbytes);            // pinned: {lines kept, junctions, junctions found}
  cnt[0] = cnt[1] = cnt[2] = 0;
  HIPCHK(c, hipMemcpyAsync(c->pin, c->io_in, fbytes, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(cnt, nl_d, 4, hipMemcpyDeviceToHost, st));
  if (want_junctions) {
    HIPCHK(c, hipMemcpyAsync(cnt + 1, nj_d, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(cnt + 2, njf_d, 4, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  if (saturation_status(c)) return 1;
  *n = rows_out(c, 0, feat);
  const int nl = cnt[0], nj = cnt[1], njf = cnt[2];
  // the reference has no junction limit (junction_detector, plnet.cpp:425-448): more than the arena holds is an ERROR, not a shorter list
  if (njf > JUNC_CAP) return fail(c, "detect_plnet: more junctions than the device arena holds (JUNC_CAP)");
  if (nl > capL || nj > capJ) return fail(c, "detect_plnet: lines / junctions do not fit the caller's buffers (capL, capJ)");
  // second (and last) round trip: the line and junction rows, whose counts are known only now, through the pinned block
  const size_t lb = (nl > 0 && lines) ? (size_t)nl * 32 : 0, jb = (nj > 0 && junc) ? (size_t)nj * AIRFE_FEAT_DIM * 4 : 0;
  if (rows_second_trip(c, {{c->d_lines, lines, lb}, {c->junc_feat, junc, jb}}, st)) return 1;
  if (nlines) *nlines = nl;
  if (njunc) *njunc = nj;
  return 0;
} AIRFE_CATCH(c)

// PLNet::infer over a device-resident batch, after the point branch ran on it (images 0 .. B-1 of the detector arena): lines of every
// image, junctions of the first nj
static int plnet_lines_batch(airfe_ctx* c, int B, int h, int w, double* d_lines, int capL, int* d_nlines, float* d_junc, int capJ,
                             int* d_njunc, int nj, int* d_found, hipStream_t st, int phase = 3) {
  if (!c->has_s0 || !c->has_s1) return fail(c, "the batched PLNet path needs the line branch (line.* in the detector pack) and cfg.plnet_s1_pack");
  if (c->prec == 2) return fail(c, "plnet_lines_batch is the 2-byte batch path (fp32 mode goes image by image: plnet_batch_f32)");
  if (B > c->Lmax) return fail(c, "batch exceeds the line-path arena");
  if (capL < 1 || !d_lines || !d_nlines) return fail(c, "detect_plnet_batch: no line output");
  if (nj < 0 || nj > B || (nj > 0 && (!d_junc || !d_njunc || capJ < 1))) return fail(c, "detect_plnet_batch: bad junction arguments");
  if ((phase & 1) && line_branch_dev(c, st, 0, B, false)) return 1;
  bool partial = false;
  if (junction_dense_maps(c, nj, capJ, phase, st, partial)) return 1;
  int* lfound = d_found ? d_found : c->d_nlines + c->Lmax;
  int* jfound = d_found ? d_found + B : c->d_njunc + c->Lmax;
  const int rc = line_tail_dev(c, 0, B, false, h, w, d_lines, capL, d_nlines, lfound, d_junc, capJ, d_njunc, jfound, nj, st, phase);
  if (partial) c->desc_dense_valid = false;       // (only the first nj images' dense maps exist)
  return rc;
}

// The batched PLNet entries in fp32 mode (cfg.precision = 2, round 6): the same results through the one-image path, image by image — the fp32 line head works
// from ONE image's fp32 conv3a activations (line_branch_dev's fused form), so every image runs encoder -> point branch -> line branch -> tail before the next
// one starts.  A correctness mode: nothing here is batched for speed.  lfound / jfound: per image "found" counts (nullptr: the context's scratch words).
static int plnet_batch_f32(airfe_ctx* c, const uint8_t* d_gray, int B, int h, int w, int stride, size_t img_stride, float* d_feat, int cap, int* d_n,
                           double* d_lines, int capL, int* d_nlines, float* d_junc, int capJ, int* d_njunc, int nj, int* lfound, int* jfound, hipStream_t st) {
  if (!c->has_s0 || !c->has_s1) return fail(c, "the batched PLNet path needs the line branch (line.* in the detector pack) and cfg.plnet_s1_pack");
  if (capL < 1 || !d_lines || !d_nlines) return fail(c, "detect_plnet_batch: no line output");
  if (nj < 0 || nj > B || (nj > 0 && (!d_junc || !d_njunc || capJ < 1))) return fail(c, "detect_plnet_batch: bad junction arguments");
  for (int b = 0; b < B; ++b) {
    const bool jn = b < nj;
    const int rc = detect_dev(c, d_gray + (size_t)b * img_stride, 1, h, w, stride, img_stride, d_feat + (size_t)b * cap * AIRFE_FEAT_DIM, cap, d_n + b, st);      // (one image: the dense NMS'd map is written)
    if (rc || line_branch_dev(c, st, 0, 1, false)) return 1;
    if (line_tail_dev(c, 0, 1, false, h, w, d_lines + (size_t)b * capL * 4, capL, d_nlines + b, lfound ? lfound + b : c->d_nlines + c->Lmax,
                      jn ? d_junc + (size_t)b * capJ * AIRFE_FEAT_DIM : nullptr, capJ, jn ? d_njunc + b : nullptr, jn ? (jfound ? jfound + b : c->d_njunc + c->Lmax) : nullptr,
                      jn ? 1 : 0, st, 3))
      return 1;
  }
  return 0;
}

int airfe_detect_plnet_batch_dev(airfe_ctx* c, const uint8_t* d_gray, int B, int h, int w, int stride, size_t img_stride, float* d_feat,
                                 int cap, int* d_n, double* d_lines, int capL, int* d_nlines, float* d_junc, int capJ, int* d_njunc,
                                 int junction_images, int* d_found, void* stream) try {
  AIRFE_ENTER(c);
  hipStream_t st = stream_of(c, stream);
  if (c->prec == 2)
    return plnet_batch_f32(c, d_gray, B, h, w, stride, img_stride, d_feat, cap, d_n, d_lines, capL, d_nlines, d_junc, capJ, d_njunc, junction_images, d_found,
                           d_found ? d_found + B : nullptr, st);
  if (detect_dev(c, d_gray, B, h, w, stride, img_stride, d_feat, cap, d_n, st)) return 1;      // (junction scores: the NMS keep plane over the raw scores, line_tail_dev)
  return plnet_lines_batch(c, B, h, w, d_lines, capL, d_nlines, d_junc, capJ, d_njunc, junction_images, d_found, st);
} AIRFE_CATCH(c)

// (d_idx == nullptr: detection only — the stereo overload of Detect without the MatchingPoints that follows it)
static int stereo_plnet_dev(airfe_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int B, int h, int w, int stride,
                            size_t img_stride, float* d_featL, float* d_featR, int cap, int* d_nL, int* d_nR, double* d_lines,
                            int capL, int* d_nlines, float* d_juncL, int capJ, int* d_njuncL, int* d_found, int32_t* d_idx,
                            float* d_score, int mcap, int* d_nmatch, hipStream_t st, const std::function<int(hipStream_t)>* after_detect = nullptr,
                            const std::function<int(hipStream_t)>* after_lines = nullptr, const LgSecondPair* x2 = nullptr) {
  if (c->prec == 2) {            // fp32 mode: image by image (plnet_batch_f32), then the matcher over the B pairs (fp32 too unless matcher_precision says otherwise)
    if (x2) return fail(c, "stereo_plnet_batch: the second (temporal) pair rides in a 2-byte forward (precision fp16 / bf16)");
    if (plnet_batch_f32(c, d_left, B, h, w, stride, img_stride, d_featL, cap, d_nL, d_lines, capL, d_nlines, d_juncL, capJ, d_njuncL, d_juncL ? B : 0, d_found,
                        d_found ? d_found + 2 * B : nullptr, st) ||
        plnet_batch_f32(c, d_right, B, h, w, stride, img_stride, d_featR, cap, d_nR, d_lines + (size_t)B * capL * 4, capL, d_nlines + B, nullptr, 0, nullptr, 0,
                        d_found ? d_found + B : nullptr, nullptr, st))
      return 1;
    if (after_detect && (*after_detect)(st)) return 1;
    if (after_lines && (*after_lines)(st)) return 1;
    if (!d_idx) return 0;
    return lightglue_dev(c, d_featL, d_nL, d_featR, d_nR, B, cap, AIRFE_FEAT_DIM, 1, 1, d_idx, d_score, mcap, d_nmatch, nullptr, st, nullptr);
  }
  if (!(2 * B <= c->Dmax))
    return fail(c, "stereo_plnet_batch: needs the one-pass stereo detector (detector + LightGlue packs loaded, 2 B <= 2 max_batch)");
  // (With stage timers on anything behind the encoder the chains run one after the other: a stage's event pair must not span the other chain.)
  const uint32_t enc_only = (1u << ST_PREPROCESS) | (1u << ST_CONV1_FUSED) | (1u << ST_CONV3X3_C64);
  const bool overlap = c->overlap_lines && (c->prof_mask & ~enc_only) == 0;
  if (detect_dev2(c, d_left, d_right, B, h, w, stride, img_stride, d_featL, d_featR, cap, d_nL, d_nR, st)) return 1;
  // lines of the 2 B images (left 0 .. B-1, right B .. 2B-1), junctions of the left ones (feature_detector.cc:100-101).
  // The line path and the matcher share nothing but the detector's results: the line path runs on the context's second stream beside
  // LightGlue on the caller's (+2 % from filled launch ramps and tails; fork behind the point branch, join behind both).  Round 2 kept this
  // off: with the line path's workgroups beside it the matcher's scores were irreproducible in ~10 % of the steps — traced in round 3 to ONE
  // packed-math instruction form in the rotary epilogue (common.h, rotate_pairs), which also failed, 50x more rarely, on one stream.
  // With that form gone: 0 deviations in 3500 overlapped and 5000 single-stream steps (profiles/r03_matcher_trace_probe1.txt, _probe2.txt).
  // after_detect (the host entry's early copy of the feature rows): on the side stream where there is one, so that it runs beside the matcher
  if (after_detect && (!d_idx || !overlap) && (*after_detect)(st)) return 1;
  // after_lines (the host entry's copy of the first line / junction rows): behind the line path, on its stream
  if (!d_idx) {
    if (plnet_lines_batch(c, 2 * B, h, w, d_lines, capL, d_nlines, d_juncL, capJ, d_njuncL, d_juncL ? B : 0, d_found, st)) return 1;
    return after_lines ? (*after_lines)(st) : 0;
  }
  if (!overlap) {
    if (plnet_lines_batch(c, 2 * B, h, w, d_lines, capL, d_nlines, d_juncL, capJ, d_njuncL, d_juncL ? B : 0, d_found, st)) return 1;
    if (after_lines && (*after_lines)(st)) return 1;
    return lightglue_dev(c, d_featL, d_nL, d_featR, d_nR, B, cap, AIRFE_FEAT_DIM, 1, 1, d_idx, d_score, mcap, d_nmatch, nullptr, st, x2);
  }
  HIPCHK(c, hipEventRecord(c->ev_fork, st));                  // behind the point branch
  HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
  int rc = 0;
  if (after_detect && (*after_detect)(c->stream2)) rc = 1;
  // The matcher is the longer chain: at small batches its launches are queued FIRST (the host needs ~4 us per launch; the ~20 launches of the line
  // path queued ahead of it kept the GPU's main queue idle for 80 us per batch-1 keyframe, tools/kf_timeline.py), at large ones the line path's
  // (there the line path is as long as the matcher and a late start would stick out behind it).
  const bool lg_first = B <= 4;
  if (!rc && lg_first) rc = lightglue_dev(c, d_featL, d_nL, d_featR, d_nR, B, cap, AIRFE_FEAT_DIM, 1, 1, d_idx, d_score, mcap, d_nmatch, nullptr, st, x2);
  if (!rc) rc = plnet_lines_batch(c, 2 * B, h, w, d_lines, capL, d_nlines, d_juncL, capJ, d_njuncL, d_juncL ? B : 0, d_found, c->stream2);
  if (!rc && after_lines && (*after_lines)(c->stream2)) rc = 1;
  if (!rc && !lg_first) rc = lightglue_dev(c, d_featL, d_nL, d_featR, d_nR, B, cap, AIRFE_FEAT_DIM, 1, 1, d_idx, d_score, mcap, d_nmatch, nullptr, st, x2);
  HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));      // (also after an error: the caller's stream never runs ahead of the side stream)
  HIPCHK(c, hipStreamWaitEvent(st, c->ev_join, 0));
  return rc;
}

int airfe_stereo_plnet_batch_dev(airfe_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int B, int h, int w, int stride,
                                 size_t img_stride, float* d_featL, float* d_featR, int cap, int* d_nL, int* d_nR, double* d_lines,
                                 int capL, int* d_nlines, float* d_juncL, int capJ, int* d_njuncL, int* d_found, int32_t* d_idx,
                                 float* d_score, int mcap, int* d_nmatch, void* stream) try {
  AIRFE_ENTER(c);
  if (!d_idx || !d_score || !d_nmatch) return fail(c, "stereo_plnet_batch: no match output");
  return stereo_plnet_dev(c, d_left, d_right, B, h, w, stride, img_stride, d_featL, d_featR, cap, d_nL, d_nR, d_lines, capL, d_nlines, d_juncL, capJ,
                          d_njuncL, d_found, d_idx, d_score, mcap, d_nmatch, stream_of(c, stream));
} AIRFE_CATCH(c)

// ONE stereo keyframe through host buffers (batch 1, the regime of AirSLAM's feature thread): what map_builder.cc:85-86 does in two façade calls —
// Detect(left, right, features, lines, junctions) = PLNet::infer twice (feature_detector.cc:97-108), then MatchingPoints(left, right) — as ONE
// queue of device work: both images go up in one copy, the detector runs over them as a batch of two, the line path of both runs on the second
// stream beside LightGlue, and everything comes back in two copies (the counted rows, then the line / junction rows whose counts are known only then).
// Per image and per pair the results are the bits the separate entries return (tests/test_gpu_keyframe.py).  match_idx == NULL: detection only.
// (track_idx != NULL: also MatchingPoints(features_last_keyframe, left_features) — map_builder.cc:96 — as the SECOND pair of the same LightGlue forward)
static int stereo_keyframe_impl(airfe_ctx* c, const uint8_t* left, const uint8_t* right, int h, int w, int stride, float* featL, float* featR, int cap,
                                int* nL, int* nR, double* linesL, double* linesR, int capL, int* nlinesL, int* nlinesR, float* juncL, int capJ,
                                int* njuncL, int32_t* match_idx, float* match_score, int mcap, int* nmatch, const float* ref_feat, int n_ref,
                                int32_t* track_idx, float* track_score, int* ntrack) {
  AIRFE_ENTER(c);
  const bool track = track_idx != nullptr;
  if (track) {
    if (!match_idx || !track_score || !ntrack) return fail(c, "stereo_keyframe_tracked: bad argument");
    if (c->Pmax < 2) return fail(c, "stereo_keyframe_tracked: needs cfg.max_batch >= 2 (two pairs per LightGlue forward)");
    if (c->mprec == 2) return fail(c, "stereo_keyframe_tracked: the temporal pair rides in a 2-byte LightGlue forward (matcher_precision fp16 / bf16)");
    if (ref_feat && (n_ref < 0 || n_ref > c->cfg.max_keypoints)) return fail(c, "stereo_keyframe_tracked: reference keypoint count exceeds max_keypoints");
    if (!ref_feat && c->ref_n < 0) return fail(c, "stereo_keyframe_tracked: no reference features were ever given");
    *ntrack = 0;
  }
  if (!left || !right || h < 1 || w < 1) return fail(c, "empty image");
  if (stride < w) return fail(c, "image stride smaller than its width");
  if (!featL || !featR || !nL || !nR || !linesL || !linesR || !nlinesL || !nlinesR || capL < 1)
    return fail(c, "stereo_keyframe: bad argument");
  if (cap < c->cfg.max_keypoints) return fail(c, "feature capacity < max_keypoints");
  const bool match = match_idx != nullptr;
  if (match && (!match_score || !nmatch || mcap < c->cfg.max_keypoints)) return fail(c, "stereo_keyframe: match buffers smaller than max_keypoints");
  const bool want_j = juncL != nullptr;
  if (want_j && (!njuncL || capJ < 1)) return fail(c, "stereo_keyframe: bad junction arguments");
  if (!(c->prec != 2 && 2 <= c->Dmax)) return fail(c, "stereo_keyframe: needs a detector arena of two images (max_batch >= 2, or detector + LightGlue packs), fp16 / bf16");
  *nL = *nR = *nlinesL = *nlinesR = 0;
  if (njuncL) *njuncL = 0;
  if (nmatch) *nmatch = 0;
  hipStream_t st = c->stream;
  const int Np = c->cfg.max_keypoints, capLd = std::min(capL, LINE_CAP), capJd = std::min(std::max(capJ, 1), JUNC_CAP);
  // device block: [counts 64 B | featL | featR | idx | score] — the part that comes back in the first copy — then [lines 2 x capLd | junctions]
  const size_t fb = (size_t)Np * AIRFE_FEAT_DIM * 4, head = 64 + 2 * fb + (size_t)Np * 24;      // (idx | score of TWO pairs: stereo, then the temporal one)
  const size_t lb = (size_t)capLd * 32, total = head + 2 * lb + (size_t)capJd * AIRFE_FEAT_DIM * 4;
  if (reserve(c, c->kf_blk, total, c->stream)) return 1;
  int* cnt = c->kf_blk.at<int>(0);                 // {nL, nR, nlines[2], -, njunc, found: lines[2] junc[1], -, nmatch: stereo, temporal}
  float *d_fL = c->kf_blk.at<float>(64), *d_fR = c->kf_blk.at<float>(64 + fb);
  int32_t* d_idx = c->kf_blk.at<int32_t>(64 + 2 * fb);
  float* d_sc = c->kf_blk.at<float>(64 + 2 * fb + (size_t)Np * 16);               // [2][Np] behind idx [2][Np][2]
  double* d_ln = c->kf_blk.at<double>(head);
  float* d_jn = c->kf_blk.at<float>(head + 2 * lb);
  // both images through the pinned block in one copy (same row pitch; the right image starts at h * stride)
  const size_t ib = (size_t)(h - 1) * stride + w, pitch = (size_t)h * stride;
  // pinned block: [counts | featL | featR] — copied back on the side stream as soon as the detector is done, beside the matcher — then the final
  // [counts] and [idx | score]
  // then, from the side stream behind the line path (also beside the matcher), the FIRST capS line rows of either image and capJS junction rows:
  // the usual keyframe (a few hundred lines and junctions) needs no second round trip for them
  const int capS = std::min(capLd, c->kf_spec_lines), capJS = want_j ? std::min(capJd, c->kf_spec_juncs) : 0;
  const size_t early = 64 + 2 * fb, late = early + 64, spec = late + (size_t)Np * 24, spec_l = (size_t)capS * 32, spec_j = (size_t)capJS * AIRFE_FEAT_DIM * 4;
  if (reserve(c, c->st_img, 2 * pitch, c->stream)) return 1;
  // (sized for the line / junction rows of the second round trip too: the block must not move between calls, a captured graph holds its address; a
  // reference on its way up sits behind everything else, 64-byte aligned)
  const size_t up_home = std::max(pitch + ib, spec + 2 * spec_l + spec_j), ref_off = (up_home + 63) / 64 * 64;
  if (ensure_pin(c, std::max(std::max(up_home, 2 * lb + (size_t)capJd * AIRFE_FEAT_DIM * 4), track && ref_feat ? ref_off + 64 + fb : 0))) return 1;
  memcpy(c->pin, left, ib);
  memcpy(c->pin + pitch, right, ib);
  const std::function<int(hipStream_t)> early_copy = [&](hipStream_t s2) -> int { return rows_home(c, c->kf_blk, early, s2); };
  // the temporal pair (last keyframe -> left image) rides in the same LightGlue forward as pair 1; its reference features live in ref_blk (uploaded
  // when given, kept otherwise: airfe_track_frame shares the block)
  LgSecondPair x2{};
  if (track) {
    if (reserve(c, c->ref_blk, 64 + fb, c->stream)) return 1;
    x2.f0 = c->ref_blk.at<const float>(64); x2.n0 = c->ref_blk.at<const int>(0);
    x2.f1 = d_fL; x2.n1 = cnt;
  }
  DrainOnError drain{c};
  const std::function<int(hipStream_t)> rows_copy = [&](hipStream_t s2) -> int {
    HIPCHK(c, hipMemcpyAsync(c->pin + spec, d_ln, spec_l, hipMemcpyDeviceToHost, s2));
    HIPCHK(c, hipMemcpyAsync(c->pin + spec + spec_l, d_ln + (size_t)capLd * 4, spec_l, hipMemcpyDeviceToHost, s2));
    if (spec_j) HIPCHK(c, hipMemcpyAsync(c->pin + spec + 2 * spec_l, d_jn, spec_j, hipMemcpyDeviceToHost, s2));
    return 0;
  };
  auto queue_all = [&]() -> int {
    drain.armed = true;
    HIPCHK(c, hipMemsetAsync(cnt, 0, 64, st));
    HIPCHK(c, hipMemcpyAsync(c->st_img.p, c->pin, pitch + ib, hipMemcpyHostToDevice, st));
    if (track && ref_feat && upload_reference(c, drain, ref_off, ref_feat, n_ref, st)) return 1;      // (never inside a capture: track runs the plain queue)
    // (match counts: cnt[10] = stereo, cnt[11] = temporal — LightGlue writes d_nmatch[pair])
    if (stereo_plnet_dev(c, c->st_img.p, c->st_img.p + pitch, 1, h, w, stride, pitch, d_fL, d_fR, Np, cnt, cnt + 1, d_ln, capLd, cnt + 2,
                         want_j ? d_jn : nullptr, capJd, want_j ? cnt + 5 : nullptr, cnt + 6, match ? d_idx : nullptr, d_sc, Np, cnt + 10, st, &early_copy, &rows_copy,
                         track ? &x2 : nullptr))
      return 1;
    // the temporal list only (map_builder.cc:96 passes true, :86 false): F-RANSAC on the device before it is copied back
    if (track && c->outlier_rejection &&
        fransac_queue(c, x2.f0, d_fL, 1, Np, d_idx + (size_t)Np * 2, d_sc + Np, Np, cnt + 11, nullptr, st))
      return 1;
    HIPCHK(c, hipMemcpyAsync(c->pin + early, cnt, 64, hipMemcpyDeviceToHost, st));
    if (match) HIPCHK(c, hipMemcpyAsync(c->pin + late, d_idx, (size_t)Np * (track ? 24 : 16) , hipMemcpyDeviceToHost, st));
    if (match && !track) HIPCHK(c, hipMemcpyAsync(c->pin + late + (size_t)Np * 16, d_sc, (size_t)Np * 4, hipMemcpyDeviceToHost, st));
    return 0;
  };
  // airfe_tuning::kf_graph = 1: the whole queue (~115 launches on two streams) is captured once per (image shape, outputs, buffers) as a hipGraph and replayed
  // with one launch — the same kernels with the same arguments, so the same bits.  The first call of a configuration runs plainly (it grows blocks and
  // sets function attributes, which a capture cannot hold), the second captures, later ones replay.  Off while stage timers or the trace are on.
  // (Measured: <= 1 % per keyframe, profiles/r04_keyframe_graph_ab.txt — the queue is bound by the GPU's ~4.7 us per dependent launch, not by the
  // host's launch calls; the default stays the plain queue.)
  KfGraph& G = c->kf_graph;
  const KfGraph::Key key{h, w, stride, capLd, capJd, want_j, match, c->pin, c->kf_blk.p, c->st_img.p};
  const bool graph_ok = c->kf_graph_on && c->prof_mask == 0 && !c->trace_on && !track;
  if (!(G.key == key)) { G.reset(); G.key = key; }
  bool replay = false;
  if (graph_ok && G.exec) {
    HIPCHK(c, hipGraphLaunch(G.exec, st));
    G.state.restore(c);
    replay = true;
  } else if (graph_ok && G.seen >= 1) {
    hipGraph_t graph = nullptr;
    HIPCHK(c, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    const int qrc = queue_all();
    const hipError_t ce = hipStreamEndCapture(st, &graph);
    if (qrc) { if (graph) (void)hipGraphDestroy(graph); return 1; }
    if (ce != hipSuccess || !graph) return fail(c, std::string("stereo_keyframe: stream capture failed: ") + hipGetErrorString(ce));
    const hipError_t ie = hipGraphInstantiate(&G.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) { G.exec = nullptr; return fail(c, std::string("stereo_keyframe: hipGraphInstantiate: ") + hipGetErrorString(ie)); }
    G.state.save(c);
    HIPCHK(c, hipGraphLaunch(G.exec, st));
    replay = true;
  } else {
    if (queue_all()) return 1;
    ++G.seen;
  }
  // the feature rows leave the pinned block while the matcher is still running (a replayed graph has no event to wait on: everything at the end)
  if (replay) HIPCHK(c, hipStreamSynchronize(st));
  else HIPCHK(c, hipEventSynchronize(c->ev_feat));
  const int n0 = *nL = rows_out(c, 0, featL), n1 = *nR = rows_out(c, 1, featR);
  if (!replay) HIPCHK(c, hipStreamSynchronize(st));
  drain.ref_uploaded = false;           // (the stream is idle: an uploaded reference is whole whatever is reported below — as airfe_track_frame does)
  if (saturation_status(c)) { *nL = *nR = 0; return 1; }
  const int* hc = reinterpret_cast<const int*>(c->pin + early);
  const int nl0 = hc[2], nl1 = hc[3], nm = std::min(hc[10], Np), nj = hc[5];
  const int fl0 = hc[6], fl1 = hc[7], fj = hc[8];
  if (match) {
    matches_out(c, late, (size_t)Np * 16, 0, nm, match_idx, match_score);
    *nmatch = (n0 > 0 && n1 > 0) ? nm : 0;                        // point_matcher.cc:53-55
  }
  if (track && n0 > 0 && c->ref_n > 0) {
    const int nt = std::min(hc[11], Np);
    matches_out(c, late, (size_t)Np * 16, Np, nt, track_idx, track_score);
    *ntrack = nt;
  }
  drain.ref_uploaded = false;           // (everything queued has completed: the reference rows are whole whatever is reported below)
  if (want_j && fj > JUNC_CAP) return fail(c, "stereo_keyframe: more junctions than the device arena holds (JUNC_CAP)");
  if (fl0 > capLd || fl1 > capLd || (want_j && fj > capJd)) return fail(c, "stereo_keyframe: lines / junctions do not fit the caller's buffers (capL, capJ)");
  const size_t b0 = (size_t)nl0 * 32, b1 = (size_t)nl1 * 32, bj = want_j ? (size_t)nj * AIRFE_FEAT_DIM * 4 : 0;
  if (nl0 <= capS && nl1 <= capS && (!want_j || nj <= capJS)) {      // the rows are already here
    if (b0) memcpy(linesL, c->pin + spec, b0);
    if (b1) memcpy(linesR, c->pin + spec + spec_l, b1);
    if (bj) memcpy(juncL, c->pin + spec + 2 * spec_l, bj);
  } else if (rows_second_trip(c, {{d_ln, linesL, b0}, {d_ln + (size_t)capLd * 4, linesR, b1}, {d_jn, juncL, bj}}, st)) return 1;
  *nlinesL = nl0; *nlinesR = nl1;
  if (njuncL) *njuncL = want_j ? nj : 0;
  drain.armed = false;
  return 0;
}

int airfe_stereo_keyframe(airfe_ctx* c, const uint8_t* left, const uint8_t* right, int h, int w, int stride, float* featL, float* featR, int cap,
                          int* nL, int* nR, double* linesL, double* linesR, int capL, int* nlinesL, int* nlinesR, float* juncL, int capJ,
                          int* njuncL, int32_t* match_idx, float* match_score, int mcap, int* nmatch) try {
  return stereo_keyframe_impl(c, left, right, h, w, stride, featL, featR, cap, nL, nR, linesL, linesR, capL, nlinesL, nlinesR, juncL, capJ, njuncL, match_idx,
                              match_score, mcap, nmatch, nullptr, 0, nullptr, nullptr, nullptr);
} AIRFE_CATCH(c)
int airfe_stereo_keyframe_tracked(airfe_ctx* c, const uint8_t* left, const uint8_t* right, int h, int w, int stride, float* featL, float* featR, int cap,
                                  int* nL, int* nR, double* linesL, double* linesR, int capL, int* nlinesL, int* nlinesR, float* juncL, int capJ,
                                  int* njuncL, int32_t* match_idx, float* match_score, int mcap, int* nmatch, const float* ref_feat, int n_ref,
                                  int32_t* track_idx, float* track_score, int* ntrack) try {
  if (c && !track_idx) return fail(c, "stereo_keyframe_tracked: no output for the temporal matches");
  return stereo_keyframe_impl(c, left, right, h, w, stride, featL, featR, cap, nL, nR, linesL, linesR, capL, nlinesL, nlinesR, juncL, capJ, njuncL, match_idx,
                              match_score, mcap, nmatch, ref_feat, n_ref, track_idx, track_score, ntrack);
} AIRFE_CATCH(c)

// ONE tracked frame through host buffers (batch 1): what map_builder.cc:94-101 does for every frame that is not a keyframe —
//     _feature_detector->Detect(image_left_rect, left_features);
//     _point_matcher->MatchingPoints(features_last_keyframe, left_features, matches, true);      (the F-RANSAC behind it stays the reference's)
// — as one queue (frame_match_host): the last keyframe's features live on the device (uploaded when ref_feat != NULL, i.e. once per keyframe, not once per
// frame), the new frame's feature rows come back on the side stream while LightGlue runs.  Bits: those of airfe_detect_points + airfe_match_lightglue.
int airfe_track_frame(airfe_ctx* c, const uint8_t* gray, int h, int w, int stride, const float* ref_feat, int n_ref, float* feat, int cap, int* n,
                      int32_t* match_idx, float* match_score, int mcap, int* nmatch) try {
  AIRFE_ENTER(c);
  if (!gray || h < 1 || w < 1) return fail(c, "empty image");
  if (stride < w) return fail(c, "image stride smaller than its width");
  if (!feat || !n || !match_idx || !match_score || !nmatch) return fail(c, "track_frame: bad argument");
  if (cap < c->cfg.max_keypoints || mcap < c->cfg.max_keypoints) return fail(c, "feature / match capacity < max_keypoints");
  if (!c->has_lg) return fail(c, "track_frame: LightGlue weights were not loaded (cfg.lightglue_pack)");
  if (c->mprec == 2 || c->prec == 2) return fail(c, "track_frame runs in fp16 / bf16");
  if (ref_feat && (n_ref < 0 || n_ref > c->cfg.max_keypoints)) return fail(c, "track_frame: reference keypoint count exceeds max_keypoints");
  *n = 0; *nmatch = 0;
  c->tk_n = -1;
  return frame_match_host(c, {"track_frame", gray, h, w, stride, &c->tk_blk, &c->ref_blk, &c->ref_n, ref_feat, n_ref, /*reject*/ true, /*sets_tk_n*/ true,
                              feat, n, match_idx, match_score, nmatch});
} AIRFE_CATCH(c)

// The promotion of map_builder.cc:104-108 (see include/airfe.h): Detect(right) + MatchingPoints(left, right) with the left rows of the last
// airfe_track_frame still on the device (the same queue; the stereo list is never outlier-rejected, the tracked frame's rows and the reference stay untouched).
int airfe_promote_frame(airfe_ctx* c, const uint8_t* right, int h, int w, int stride, float* featR, int cap, int* nR, int32_t* match_idx,
                        float* match_score, int mcap, int* nmatch) try {
  AIRFE_ENTER(c);
  if (!right || h < 1 || w < 1) return fail(c, "empty image");
  if (stride < w) return fail(c, "image stride smaller than its width");
  if (!featR || !nR || !match_idx || !match_score || !nmatch) return fail(c, "promote_frame: bad argument");
  if (cap < c->cfg.max_keypoints || mcap < c->cfg.max_keypoints) return fail(c, "feature / match capacity < max_keypoints");
  if (!c->has_lg) return fail(c, "promote_frame: LightGlue weights were not loaded (cfg.lightglue_pack)");
  if (c->mprec == 2 || c->prec == 2) return fail(c, "promote_frame runs in fp16 / bf16");
  if (c->tk_n < 0 || !c->tk_blk.p) return fail(c, "promote_frame: no airfe_track_frame preceded it (the left features live on the device since that call)");
  *nR = 0; *nmatch = 0;
  return frame_match_host(c, {"promote_frame", right, h, w, stride, &c->pr_blk, &c->tk_blk, &c->tk_n, nullptr, 0, /*reject*/ false, /*sets_tk_n*/ false,
                              featR, nR, match_idx, match_score, nmatch});
} AIRFE_CATCH(c)

int airfe_adopt_reference(airfe_ctx* c) try {
  AIRFE_ENTER(c);
  if (c->tk_n < 0 || !c->tk_blk.p) return fail(c, "adopt_reference: no airfe_track_frame preceded it");
  const size_t fb = (size_t)c->cfg.max_keypoints * AIRFE_FEAT_DIM * 4;
  if (reserve(c, c->ref_blk, 64 + fb, c->stream)) return 1;
  // [count | rows] have the same layout in both blocks (the count's word 0; words 1.. of the header are scratch of the entries)
  HIPCHK(c, hipMemcpyAsync(c->ref_blk.p, c->tk_blk.p, 64 + (size_t)std::max(c->tk_n, 0) * AIRFE_FEAT_DIM * 4, hipMemcpyDeviceToDevice, c->stream));
  c->ref_n = c->tk_n;
  return 0;
} AIRFE_CATCH(c)

}  // extern "C"
