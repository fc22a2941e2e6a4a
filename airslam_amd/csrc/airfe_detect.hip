// airfe — the detector pipeline (encoder, heads, NMS, top-K, descriptors) on the device (see airfe_host.h)
#include "airfe_host.h"

namespace airfe_host {

int ensure_tables(airfe_ctx* c, int h, int w) {
  if (c->tab_w == w && c->tab_h == h) return 0;
  const auto xt = resize_table(AIRFE_INTERNAL_SIZE, w), yt = resize_table(AIRFE_INTERNAL_SIZE, h);
  // the image size changed: a pre-process of the previous size may still be reading the tables on a CALLER's stream (the *_dev entry
  // points), so the whole device is drained before they are rewritten — once per size change, not per call
  if (c->tab_w != -1) HIPCHK(c, hipDeviceSynchronize());   // (-1: no table yet, nothing can be reading it)
  HIPCHK(c, hipMemcpyAsync(c->xtab, xt.data(), xt.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->ytab, yt.data(), yt.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // host vectors go out of scope
  c->tab_w = w;
  c->tab_h = h;
  return 0;
}

int run_conv(airfe_ctx* c, const ConvW& w, const uint16_t* x, uint16_t* y, int B, int H, int W, int pool, int out_pad,
             hipStream_t st) {
  ConvArgs a;
  a.X = x; a.Wp = w.w; a.bias = w.b; a.Y = y;
  a.B = B; a.H = H; a.W = W; a.CIN = w.cin; a.COUT = w.cout;
  a.pool = pool; a.out_pad = out_pad; a.relu = 1;
  const double px = (double)B * H * W;
  const double ob = px / (pool ? 4 : 1) * w.cout * 2;
  {
    ProfScope ps(c, w.cin == 64 ? ST_CONV3X3_C64 : ST_CONV3X3_C128, st, 2.0 * px * w.cin * w.cout * 9,
                 px * w.cin * 2 + ob + 9.0 * w.cin * w.cout * 2);
    launch_conv3x3(c->prec, a, st);
  }
  return c->cfg.check_launches ? launch_status(c) : 0;       // (without the flag: once per pipeline, at its end)
}

// ---- fp32 correctness path: the SuperPoint-VGG encoder + heads up to the dense logits / descriptor maps (what follows — soft-max,
// NMS, top-K, descriptor sampling — is fp32 in every mode and shared)
void f32_conv(const airfe_ctx::F32Conv& w, const float* x, float* y, int B, int H, int W, int opad, hipStream_t st) {
  launch_conv3x3_f32(x, w.w, w.b, y, B, H, W, w.cin, w.cout, opad, st);
}
int encode_f32(airfe_ctx* c, const uint8_t* d_gray, int B, int h, int w, int stride, size_t img_stride, hipStream_t st) {
  const int R = AIRFE_INTERNAL_SIZE;
  for (int c0 = 0; c0 < B; c0 += c->f_B) {
    const int cb = std::min(c->f_B, B - c0);
    launch_preprocess(d_gray + (size_t)c0 * img_stride, cb, h, w, stride, img_stride, c->xtab, c->ytab, c->lut, c->img32, R, R, st);
    launch_conv1a_f32(c->img32, c->c1a_w, c->c1a_b, c->f1a, cb, R, R, st);
    f32_conv(c->f_c1b, c->f1a, c->f1b, cb, R, R, 1, st);
    launch_maxpool2_f32(c->f1b, c->fp1, cb, R, R, 64, st);
    f32_conv(c->f_c2a, c->fp1, c->f2a, cb, R / 2, R / 2, 1, st);
    f32_conv(c->f_c2b, c->f2a, c->f2b, cb, R / 2, R / 2, 1, st);
    launch_maxpool2_f32(c->f2b, c->fp2, cb, R / 2, R / 2, 64, st);
    f32_conv(c->f_c3a, c->fp2, c->f3a, cb, R / 4, R / 4, 1, st);
    f32_conv(c->f_c3b, c->f3a, c->f3b, cb, R / 4, R / 4, 1, st);
    launch_maxpool2_f32(c->f3b, c->fp3, cb, R / 4, R / 4, 128, st);
    f32_conv(c->f_c4a, c->fp3, c->f4a, cb, R / 8, R / 8, 1, st);
    f32_conv(c->f_c4b, c->f4a, c->f4b, cb, R / 8, R / 8, 1, st);
    f32_conv(c->f_cPa, c->f4b, c->fPa, cb, R / 8, R / 8, 0, st);
    f32_conv(c->f_cDa, c->f4b, c->fDa, cb, R / 8, R / 8, 0, st);
    const int cells = cb * (R / 8) * (R / 8);
    const size_t cell0 = (size_t)c0 * (R / 8) * (R / 8);
    GemmF32Args g;
    g.X1 = c->fPa; g.ld1 = 256; g.K1 = 256; g.K = 256; g.W = c->f_cPb.w; g.bias = c->f_cPb.b; g.M = cells; g.N = 65;
    g.Y = c->logits + cell0 * 72; g.ldy = 72;
    launch_gemm_f32(g, st);
    g.X1 = c->fDa; g.W = c->f_cDb.w; g.bias = c->f_cDb.b; g.N = 256; g.Y = c->desc + cell0 * 256; g.ldy = 256;
    launch_gemm_f32(g, st);
  }
  launch_softmax_d2s(c->logits, 72, c->heat, B, R / 8, R / 8, st);
  c->desc_normalised = false;
  return launch_status(c);
}

// convDb over every cell of the batch -> c->desc [B][64][64][256] fp32, un-normalised
int dense_desc_head(airfe_ctx* c, int B, hipStream_t st) {
  const int R = AIRFE_INTERNAL_SIZE, cells = B * (R / 8) * (R / 8);
  GemmArgs g;
  g.X1 = c->aDa; g.ld1 = 256; g.K1 = 256; g.Wp = c->cDb.w; g.bias = c->cDb.b;
  g.M = cells; g.N = 256; g.cb_total = c->cDb.cbt; g.epi = EPI_STORE_F32; g.out = c->desc; g.ldo = 256;
  g.small_max = c->gemm_small_max; g.g8_min = c->gemm8_min; g.gr_min = c->gemmr_min; g.gr_wgs = c->gemmr_wgs;
  {
    ProfScope ps(c, ST_HEAD_GEMM, st, 2.0 * cells * 256 * 256, (double)cells * (512 + 1024));
    // large batches (round 6): 512 B in and 1 KB of fp32 out per cell is HBM work — the tiled kernel ran it at 1.8 TB/s (225 us per 64 images); the streaming kernel's
    // identity-index form (kernels_gemmr.hip) has the same fragments, K order and bias placement: the same bits
    if (c->desc_gather_stream && cells >= c->gemmr_min && gemmr_gather_applicable(256, g)) launch_gemmr_gather(c->prec, g, st);
    else launch_gemm(c->prec, 256, false, g, st);
  }
  // F.normalize of the dense map is applied lazily: sample_desc_kernel normalises just the 4 taps each keypoint reads
  // (same operations, same bits) — a dense pass moved 8 MB/image to serve 400 x 4 cell reads.
  c->desc_normalised = false;
  return c->cfg.check_launches ? launch_status(c) : 0;
}

// The descriptor head convDb (1x1, 256 -> 256) is only ever READ at the <= 4 cells each keypoint samples: large batches (sparse) run it as a
// gather GEMM over those rows after the top-K (detect_tail_dev) — 1600 of 4096 cells per image at 400 keypoints, and 1.6 instead of 4 MB
// of fp32 written.  The dense map stays for small batches (the batch-1 line path samples junction descriptors from it) and
// for the inspection hook, which rebuilds it on demand.  Same kernel, same K order: the rows are bit-identical either way.
// The decision, the dense head where it runs and the context's record of it; shared by detect_dev2 and the test hook airfe_debug_detector_tail.
int point_desc_head(airfe_ctx* c, int B, int cap, hipStream_t st, bool& sparse) {
  const int R = AIRFE_INTERNAL_SIZE;
  sparse = B > 2 && cap * 4 <= (R / 8) * (R / 8) && cap <= 1024;
  if (!sparse && dense_desc_head(c, B, st)) return 1;
  c->desc_dense_valid = !sparse;
  c->last_B = B;
  return 0;
}

// Everything of the detector behind the score head, over the B images whose score maps are in c->heat and whose convDa activations are in c->aDa: NMS, candidate
// compaction, top-K, descriptor head over the sampled cells (sparse_desc; else the dense map is already in c->desc) and descriptor sampling.  two: images
// b >= Bs write the second destination.  Shared by detect_dev2 and the test hook airfe_debug_detector_tail (airfe_debug.hip), so that hand-built score maps run
// the very launches production runs.
int detect_tail_dev(airfe_ctx* c, int B, int Bs, bool two, bool sparse_desc, int h, int w, float* d_feat, float* d_feat1, int cap, int* d_n, int* d_n1,
                    hipStream_t st) {
  const int R = AIRFE_INTERNAL_SIZE;
  const int ccap = R * R;
  {
    ProfScope ps(c, ST_NMS, st, 0, (double)B * R * R * 8);
    if (c->cfg.nms_radius == 4) {                        // the reference's radius: simple_nms in registers (kernels_nms512.hip; R = 512)
      // the dense NMS'd map is consumed only by the batch-1 line path (junction scores) and the inspection hook: large batches skip
      // its 1 MB / image write (airfe_debug_detector_maps rebuilds it on demand; the batched junction scores come from the keep plane, line_tail_dev)
      c->nms_map_valid = B <= 2;
      launch_nms512_candidates(c->heat, c->nms_map_valid ? c->heat_nms : nullptr, c->nms_mask, B, c->cfg.keypoint_threshold,
                               c->cfg.remove_borders, c->cand, c->cand_cnt, ccap, st);
    } else if (c->cfg.nms_radius > 0) {
      c->nms_map_valid = true;
      launch_simple_nms(c->heat, c->heat_nms, c->nms_tmp, B, R, R, c->cfg.nms_radius, st);
      launch_candidates(c->heat_nms, B, R, R, c->cfg.keypoint_threshold, c->cfg.remove_borders, c->cand, c->cand_cnt, ccap, st);
    } else {
      launch_candidates(c->heat, B, R, R, c->cfg.keypoint_threshold, c->cfg.remove_borders, c->cand, c->cand_cnt, ccap, st);
    }
  }
  // The two feature destinations of a stereo batch: ONE launch of every kernel below over the 2 Bs images, which pick their destination by image index
  // (one-destination calls pass no second set).
  const int M = B * cap * 4, Mp = (M + 255) / 256 * 256;
  {
    ProfScope ps(c, ST_SELECT, st, 0, (double)B * 8192 * 8);
    SelectExtra ex;
    if (two) { ex.feat1 = d_feat1; ex.n_out1 = d_n1; ex.Bs = Bs; }
    // sparse descriptors: the top-K kernel also writes the four head rows each slot will sample (the gather GEMM's row list; zero for slots k >= n)
    if (sparse_desc) { ex.desc_idx = c->desc_idx; ex.HC = R / 8; ex.WC = R / 8; }
    launch_select_list(c->cand, c->cand_cnt, ccap, B, R, c->cfg.max_keypoints, cap, d_feat, d_n, st, &ex);
  }
  bool sampled = false;
  if (sparse_desc) {
    if (Mp > M) HIPCHK(c, hipMemsetAsync(c->desc_idx + M, 0, (size_t)(Mp - M) * 4, st));
    GemmArgs g;
    g.X1 = c->aDa; g.ld1 = 256; g.K1 = 256; g.Wp = c->cDb.w; g.bias = c->cDb.b; g.rowidx = c->desc_idx;
    g.M = Mp; g.N = 256; g.cb_total = c->cDb.cbt; g.epi = EPI_STORE_F32; g.out = c->desc; g.ldo = 256;
    g.gr_wgs = c->gemmr_wgs;
    // large batches: the streaming kernel with gathered rows (kernels_gemmr.hip, GATHER) — the tiled 8-wave kernel ran this HBM-bound shape at 2.3 TB/s; the same bits.
    // Its SAMPLE form finishes the keypoints from the tile in LDS: no head rows written (1 KB per row) and read back, no sampling launch.
    const bool stream = c->desc_gather_stream && Mp >= c->gemmr_min && gemmr_gather_applicable(256, g);
    if (stream && gemmr_gather_sample_applicable(g)) {
      ProfScope ps(c, ST_HEAD_GEMM, st, 2.0 * Mp * 256 * 256, (double)Mp * 512 + (double)B * c->cfg.max_keypoints * 1036);
      DescSample ds;
      ds.feat = d_feat; ds.n = d_n; ds.feat1 = two ? d_feat1 : nullptr; ds.n1 = two ? d_n1 : nullptr; ds.Bs = two ? Bs : B; ds.B = B; ds.cap = cap;
      ds.HC = R / 8; ds.WC = R / 8; ds.w_scale = (float)w / (float)R; ds.h_scale = (float)h / (float)R; ds.flag = c->sat_flag;
      launch_gemmr_gather_sample(c->prec, g, ds, st);
      sampled = true;
    } else {
      ProfScope ps(c, ST_HEAD_GEMM, st, 2.0 * Mp * 256 * 256, (double)Mp * (512 + 1024));
      if (stream) launch_gemmr_gather(c->prec, g, st);
      else launch_gemm8(c->prec, 256, false, g, st);
    }
  }
  if (!sampled) {
    ProfScope ps(c, ST_SAMPLE, st, 0, (double)B * c->cfg.max_keypoints * (4096 + 1036));
    launch_sample_desc(c->desc, B, R / 8, R / 8, d_feat, d_n, cap, (float)w / (float)R, (float)h / (float)R,
                       sparse_desc ? 1 : (c->desc_normalised ? 0 : 1), st, sparse_desc ? 1 : 0, c->sat_flag, two ? d_feat1 : nullptr, two ? d_n1 : nullptr, Bs);
  }
  return launch_status(c);
}

// Detector over ONE batch of B images, or — d_gray1 != nullptr — over the 2 B images of B stereo pairs in one pass (images 0 .. B-1 from
// d_gray, B .. 2B-1 from d_gray1; features to d_feat / d_feat1): every whole-batch kernel then runs once over twice the tiles instead
// of twice (half the launches, prologues and tails of the second half of the network; per-image results do not depend on the batch).
int detect_dev2(airfe_ctx* c, const uint8_t* d_gray, const uint8_t* d_gray1, int Bs, int h, int w, int stride, size_t img_stride,
                float* d_feat, float* d_feat1, int cap, int* d_n, int* d_n1, hipStream_t st) {
  if (!c->has_sp) return fail(c, "detector weights were not loaded (cfg.superpoint_pack)");
  const int B = d_gray1 ? 2 * Bs : Bs;
  if (Bs < 1 || Bs > c->Bmax || B > c->Dmax) return fail(c, "batch exceeds cfg.max_batch");
  if (h < 1 || w < 1) return fail(c, "empty image");
  if (cap < c->cfg.max_keypoints) return fail(c, "feature capacity < max_keypoints");
  if (ensure_tables(c, h, w)) return 1;
  const int R = AIRFE_INTERNAL_SIZE;
  bool sparse_desc = false;
  if (c->prec == 2) {
    if (d_gray1) return fail(c, "detect_dev2: the fp32 path takes one source");
    if (encode_f32(c, d_gray, B, h, w, stride, img_stride, st)) return 1;
  } else {
    for (int c0 = 0, cb = 0; c0 < B; c0 += cb) {
      cb = std::min(c->chunk, B - c0);
      {                                                                  // a chunk may straddle the two sources: still one pre-process launch
        ProfScope ps(c, ST_PREPROCESS, st, 0, (double)cb * ((double)h * w + (double)R * R * 4));
        const int n0 = std::min(std::max(Bs - c0, 0), cb);              // images of this chunk that come from d_gray
        const uint8_t* s0 = n0 > 0 ? d_gray + (size_t)c0 * img_stride : nullptr;
        const uint8_t* s1 = cb > n0 ? d_gray1 + (size_t)(c0 + n0 - Bs) * img_stride : nullptr;
        launch_preprocess(s0 ? s0 : s1, cb, h, w, stride, img_stride, c->xtab, c->ytab, c->lut, c->img32, R, R, st, s0 ? s1 : nullptr, n0);
      }
      {
        // conv1a (Cin = 1) fused into the persistent conv1b kernel: its 64-channel full-resolution output never
        // reaches HBM (kernels_conv64r.hip).  FLOPs/bytes below are the algorithmic ones of conv1a + conv1b.
        ConvArgs a;
        a.Wp = c->c1b.w; a.bias = c->c1b.b; a.Y = c->a1b; a.B = cb; a.H = R; a.W = R; a.CIN = 64; a.COUT = 64;
        a.pool = 1; a.out_pad = 1; a.relu = 1;
        a.img = c->img32; a.w1a = c->c1a_w; a.b1a = c->c1a_b;
        const double px = (double)cb * R * R;
        ProfScope ps(c, ST_CONV1_FUSED, st, 2.0 * px * 9 * 64 + 2.0 * px * 64 * 64 * 9, px * 4 + px / 4 * 128 + 9.0 * 64 * 64 * 2);
        launch_conv64r(c->prec, a, st);
      }
      if (run_conv(c, c->c2a, c->a1b, c->a2a, cb, R / 2, R / 2, 0, 1, st)) return 1;
      if (run_conv(c, c->c2b, c->a2a, c->a2b + (size_t)c0 * (R / 4 + 2) * (R / 4 + 2) * 64, cb, R / 2, R / 2, 1, 1, st)) return 1;
    }
    if (run_conv(c, c->c3a, c->a2b, c->a3a, B, R / 4, R / 4, 0, 1, st)) return 1;
    if (run_conv(c, c->c3b, c->a3a, c->a3b, B, R / 4, R / 4, 1, 1, st)) return 1;
    if (run_conv(c, c->c4a, c->a3b, c->a4a, B, R / 8, R / 8, 0, 1, st)) return 1;
    if (run_conv(c, c->c4b, c->a4a, c->a4b, B, R / 8, R / 8, 0, 1, st)) return 1;
    if (run_conv(c, c->cPa, c->a4b, c->aPa, B, R / 8, R / 8, 0, 0, st)) return 1;
    if (run_conv(c, c->cDa, c->a4b, c->aDa, B, R / 8, R / 8, 0, 0, st)) return 1;
    const int cells = B * (R / 8) * (R / 8);
    {
      GemmArgs g;
      g.X1 = c->aPa; g.ld1 = 256; g.K1 = 256; g.Wp = c->cPb.w; g.bias = c->cPb.b;
      g.M = cells; g.N = 65; g.cb_total = c->cPb.cbt; g.epi = EPI_STORE_F32; g.out = c->logits; g.ldo = 72;
      g.small_max = c->gemm_small_max; g.g8_min = c->gemm8_min; g.gr_min = c->gemmr_min; g.gr_wgs = c->gemmr_wgs;
      // soft-max + depth-to-space in the GEMM's epilogue, at EVERY batch size (one summation order): no logits in memory
      g.epi = EPI_SOFTMAX_D2S; g.out = c->heat; g.d2s_hc = R / 8; g.d2s_wc = R / 8; g.flag = c->sat_flag;
      ProfScope ps(c, ST_HEAD_GEMM, st, 2.0 * cells * 256 * 65, (double)cells * (512 + 256));
      launch_gemm8(c->prec, 256, false, g, st);
    }
    if (point_desc_head(c, B, cap, st, sparse_desc)) return 1;
  }
  return detect_tail_dev(c, B, Bs, d_gray1 != nullptr, sparse_desc, h, w, d_feat, d_feat1, cap, d_n, d_n1, st);
}

int detect_dev(airfe_ctx* c, const uint8_t* d_gray, int B, int h, int w, int stride, size_t img_stride, float* d_feat,
               int cap, int* d_n, hipStream_t st) {
  return detect_dev2(c, d_gray, nullptr, B, h, w, stride, img_stride, d_feat, nullptr, cap, d_n, nullptr, st);
}

}  // namespace airfe_host
