// airfe — the PLNet line path on the device: its steps, each launch sequence stated once, and the compositions of them that production runs (see airfe_host.h)
#include "airfe_host.h"

namespace airfe_host {

// get_junctions over c->l_jloc / c->l_joff of stage slots 0 .. nb-1: top-300 of the 3x3-suppressed junction map (score descending, raster ascending on ties) -> juncs_pred
// in the stage blocks.  Shared by line_branch_dev and the test hook airfe_debug_junctions_topk.
void junctions_topk_dev(airfe_ctx* c, int nb, hipStream_t st) {
  const int F = 128, ccap = F * F;
  launch_candidates_nms3(c->l_jloc, nb, F, F, 1e-30f, c->l_cand, c->l_cand_cnt, ccap, st);      // non_maximum_suppression (3x3) inside the compaction
  SelectExtra jx;
  jx.sort_all = 1;                  // fewer than 300 maxima (a flat-topped or saturated jloc): still score order, as the contract's top-k — not detect_point's raster rule
  launch_select_list(c->l_cand, c->l_cand_cnt, ccap, nb, F, 300, 320, c->l_sel, c->l_nsel, st, &jx);
  launch_s0_juncs(c->l_sel, c->l_nsel, c->l_joff, c->s0_stage + SG_JUNCS, 300, 320, nb, SG_STRIDE, st);
}

// ---- The steps of the PLNet line path over stage slots 0 .. nb-1.  Each launch sequence is stated here once: line_branch_dev, line_tail_dev and line_post_dev
// compose the steps, and the test hooks (airfe_debug.hip, airfe_debug_plnet_s1) call the same steps between their staging and their read-back, with the few
// values a hook varies as parameters (tests/test_line_path_one_statement_cpu.py keeps it so).

// The 1x1 line head over c->l_feat as a GEMM.  fused: all 145 channels -> c->l_head [128*128][160]; else the 17 decoded channels -> c->l_dec [nb][128*128][32].
void line_head_gemm(airfe_ctx* c, int nb, bool fused, int prec, const LinW& hw, hipStream_t st) {
  const int F = 128;
  GemmArgs g;
  g.X1 = c->l_feat; g.ld1 = 128; g.K1 = 128; g.Wp = hw.w; g.bias = hw.b;
  g.M = nb * F * F; g.N = hw.N; g.cb_total = hw.cbt; g.epi = EPI_STORE_F32; g.out = fused ? c->l_head : c->l_dec; g.ldo = fused ? 160 : 32;
  g.small_max = c->gemm_small_max; g.g8_min = c->gemm8_min; g.gr_min = c->gemmr_min; g.gr_wgs = c->gemmr_wgs;
  if (!fused) g.small_max = 1 << 30;      // one 64-feature block: the no-LDS kernel computes 64 columns per row instead of the tiled kernels' 256
  ProfScope ps(c, ST_HEAD_GEMM, st, 2.0 * nb * F * F * 128 * hw.N, (double)nb * F * F * (256 + 4.0 * g.ldo));
  launch_gemm(prec, 128, false, g, st);
}

// The 17-channel head and its decode in one pass over the line features (kernels_s0.hip): lines_pred, jloc, joff, the pixel-major thin | aux (and jnms where asked).
void line_head_decode(airfe_ctx* c, int nb, int prec, const LinW& hw, float* jnms, int wgs, hipStream_t st) {
  const int F = 128;
  ProfScope ps(c, ST_PL_DECODE, st, 2.0 * nb * F * F * 128 * 17, (double)nb * F * F * (256 + 92));
  launch_s0_head_decode(prec, c->l_feat, hw.w, hw.b, c->s0_stage + SG_LP, c->l_jloc, jnms, c->l_joff, c->l_ta8, nb, SG_STRIDE, st, wgs);
}

// The decode over head rows of layout (ld, off) — (160, 128): line_head_gemm's fused rows, (32, 0): its 17-channel rows.  ta8 / loi_chw: also the pixel-major
// thin | aux copy / the contract's CHW loi_features of slot 0 (c->s0_loi; the (160, 128) layout only).
void line_decode_rows(airfe_ctx* c, int nb, const float* head, int ld, int off, float* jnms, bool ta8, bool loi_chw, hipStream_t st) {
  float* d = c->s0_stage;
  launch_s0_decode(head, ld, off, d + SG_LP, c->l_jloc, jnms, c->l_joff, d + SG_THIN, d + SG_AUX, loi_chw ? c->s0_loi : nullptr, ta8 ? c->l_ta8 : nullptr, nb,
                   SG_STRIDE, st);
}

// The junction-to-line match (exact_all: every proposal against every junction, the inspection hook's export).  Leaves c->wf_counted for line_dedup.
void line_match(airfe_ctx* c, int nb, bool exact_all, hipStream_t st) {
  float* d = c->s0_stage;
  c->wf_counted = launch_s0_j2l(d + SG_LP, d + SG_JUNCS, 300, KEEP_CAP, 10.0f, d + SG_KEEP, d + SG_MIN, d + SG_MAX, c->wf_counts, nb, SG_STRIDE, exact_all ? 1 : 0, st);
}

// wireframe_matcher: the kept list and the unique junction pairs.  Consumes c->wf_counted.
void line_dedup(airfe_ctx* c, int nb, hipStream_t st) {
  float* d = c->s0_stage;
  launch_wireframe(d + SG_KEEP, d + SG_MIN, d + SG_MAX, KEEP_CAP, 300, c->wf_table, c->wf_keep, c->wf_pairs, c->wf_rep, KEEP_CAP, LINE_CAP,
                   c->wf_counts, c->wf_counted, d + SG_JUNCS, d + SG_LP, c->s1_la, c->wf_prop, nb, SG_STRIDE, st);
  c->wf_counted = false;
}

// The four bilinear tap rows of every junction -> c->l_ridx, zero-padded to the gather GEMM's 256-row multiple.
int line_tap_rows(airfe_ctx* c, int nb, hipStream_t st) {
  const int M = nb * 1200, Mp = (M + 255) / 256 * 256;
  launch_s1_junc_rows(c->s0_stage + SG_JUNCS, 300, c->l_ridx, nb, SG_STRIDE, st);
  if (Mp > M) HIPCHK(c, hipMemsetAsync(c->l_ridx + M, 0, (size_t)(Mp - M) * 4, st));
  return 0;
}

// The LOI head at the tap rows only: c->l_ridx -> c->l_lrows [nb * 1200][128].
void line_loi_rows(airfe_ctx* c, int nb, hipStream_t st) {
  const int M = nb * 1200, Mp = (M + 255) / 256 * 256;
  GemmArgs g;
  g.X1 = c->l_feat; g.ld1 = 128; g.K1 = 128; g.Wp = c->cLh_loi.w; g.bias = c->cLh_loi.b; g.rowidx = c->l_ridx;
  g.M = Mp; g.N = 128; g.cb_total = c->cLh_loi.cbt; g.epi = EPI_STORE_F32; g.out = c->l_lrows; g.ldo = 128;
  g.gr_wgs = c->gemmr_wgs;
  // large batches: the streaming kernel with gathered rows (kernels_gemmr.hip, K = N = 128 form) — the tiled kernel ran this HBM-bound shape at 0.8 TB/s; the same bits
  if (c->desc_gather_stream && Mp >= c->gemmr_min && c->prec != 2 && gemmr_gather128_applicable(g)) launch_gemmr_gather128(c->prec, g, st);
  else launch_gemm8(c->prec, 128, false, g, st);
}

// The junction projection and stage 1 in one of the forms S1Form names (airfe_host.h).  wgs: stage 1's workgroups (0 = the launcher's rule).
void line_stage1(airfe_ctx* c, int nb, int form, int wgs, hipStream_t st) {
  float* d = c->s0_stage;
  const bool chw = form == S1_CHW, rows = form == S1_ROWS || form == S1_ROWS_H, pairs = form == S1_ROWS_H || form == S1_HEAD_H;
  if (form == S1_ROWS_H) launch_s1h_junc_proj(d + SG_JUNCS, c->l_lrows, 300, c->s1_wsplit[4], c->s1_wsplit[5], c->s1_jfeat, nb, SG_STRIDE, st);
  else if (!chw)
    launch_s1_junc_proj(d + SG_JUNCS, rows ? nullptr : c->l_head, rows ? 0 : (size_t)128 * 128 * 160, rows ? 0 : 160, rows ? c->l_lrows : nullptr, 300, c->s1_w[0],
                        c->s1_jfeat, nb, SG_STRIDE, st);
  if (pairs)      // the four dense layers on the 2-byte matrix pipe, operands as fp16 (hi, lo) pairs: fp32-accurate (kernels_ext.hip)
    launch_plnet_s1h(c->wf_pairs, c->wf_counts, c->s1_jfeat, c->l_ta8, c->s1_wsplit, c->s1_w, c->s1_la, c->wf_prop, c->s1_sc, LINE_CAP, nb, st, wgs);
  else            // (chw: all 496 features per line from the CHW block, no projection)
    launch_plnet_s1(d + SG_JUNCS, d + SG_LP, c->wf_keep, c->wf_pairs, c->wf_rep, c->wf_counts, chw ? c->s0_loi : nullptr, 0, chw ? nullptr : c->s1_jfeat,
                    chw ? nullptr : c->l_ta8, d + SG_THIN, d + SG_AUX, c->s1_w, c->s1_la, c->s1_sc, KEEP_CAP, LINE_CAP, nb, SG_STRIDE, st, wgs);
}

// PLNet stage-0 LINE branch of images [i0, i0 + nb) of the batch the detector just ran on: fills stage slots 0 .. nb-1 with the Appendix
// A.1 tensors in the contract's own layouts, so that everything downstream (wireframe dedup, stage 1, filters) is the code the golden
// tests pin.  chw: also the contract's CHW loi_features of slot 0 (the inspection hook; the line path samples the head rows directly).
int line_branch_dev(airfe_ctx* c, hipStream_t st, int i0, int nb, bool chw) {
  if (!c->has_s0) return fail(c, "the detector pack carries no line branch (line.* tensors)");
  if (!c->s0_stage) return fail(c, "the line path arena is not allocated (cfg.plnet_s1_pack)");
  if (nb < 1 || nb > c->Lmax || i0 < 0 || i0 + nb > c->Dmax) return fail(c, "line branch: image range outside the arena");
  const int F = 128;
  // Two forms of the 1x1 head.  FUSED (fp32 mode, inspection hook; one image): all 145 channels at every pixel -> l_head [128*128][160].
  // SPLIT (everything else): the 17 decoded channels at every pixel, decoded in the same pass (or, airfe_tuning::fuse_dec = 0, -> l_dec [nb][128*128][32]
  // and a decode pass of its own); the 128 LOI channels — read only at the four
  // bilinear taps of the <= 300 junctions — by a gather GEMM over those <= 1200 rows per image once the junctions are known (line_tail_dev):
  // the fused head wrote 1.07 GB of LOI features per 128 images to read 7 % of them.  Same kernel, same K order: the same bits.
  const bool fused = c->prec == 2 || chw;
  if (fused && (nb != 1 || i0 != 0)) return fail(c, "the fused line head (fp32 mode, inspection hook) runs one image at a time");
  c->line_sparse = !fused;
  bool head_done = false;
  if (c->prec == 2) {
    launch_conv3x3_f32(c->f3a, c->f_cL1.w, c->f_cL1.b, c->fL1, 1, F, F, 128, 128, 0, st);
    GemmF32Args g;
    g.X1 = c->fL1; g.ld1 = 128; g.K1 = 128; g.K = 128; g.W = c->f_cLh.w; g.bias = c->f_cLh.b; g.M = F * F; g.N = 145; g.Y = c->l_head; g.ldy = 160;
    launch_gemm_f32(g, st);
  } else {
    // conv3a features (zero-bordered NHWC, still in the arena for the whole batch) -> [nb * 128*128][128]
    if (run_conv(c, c->cL1, c->a3a + (size_t)i0 * (F + 2) * (F + 2) * 128, c->l_feat, nb, F, F, 0, 0, st)) return 1;
    head_done = !fused && c->fuse_dec;
    if (head_done) line_head_decode(c, nb, c->prec, c->cLh_dec, nullptr, 0, st);
    else line_head_gemm(c, nb, fused, c->prec, fused ? c->cLh : c->cLh_dec, st);
  }
  {
    // head rows read once, 49152 proposals + maps written; the j2l match reads them again
    ProfScope ps(c, ST_PL_DECODE, st, 0, (double)nb * (128.0 * 128 * (17 * 4 + 3 * 16 + 11 * 4) + 3.0 * 49152 * (16 + 12)));
    // (head_done: lines_pred, jloc, jnms, joff and the pixel-major thin | aux are already there)
    if (!head_done) line_decode_rows(c, nb, fused ? c->l_head : c->l_dec, fused ? 160 : 32, fused ? 128 : 0, nullptr, true, chw, st);
    junctions_topk_dev(c, nb, st);
    line_match(c, nb, chw, st);
  }
  return launch_status(c);
}

// The junction tail without the byte maps and without a dense descriptor map: the junction list inside the line filter (launch_line_filter_junc) and the descriptor
// head at the junctions' tap rows with the sampling in its epilogue (launch_gemmr_gather_sample_junc).  It runs where the batched entries leave no dense maps — radius-4
// NMS with the keep plane alone, no dense descriptor map — and the streaming gather GEMM applies at capJ * nj slots; everywhere else (B <= 2: the batch-1 keyframe path,
// other radii, fp32 mode, the inspection hooks) the byte-map launches and sample_desc run as before.
static void junction_gemm_args(airfe_ctx* c, int i0, int nj, float* d_junc, int capJ, const int* d_njunc, int h, int w, GemmArgs& g, DescSample& ds) {
  const int R = AIRFE_INTERNAL_SIZE;
  g.X1 = c->aDa + (size_t)i0 * (R / 8) * (R / 8) * 256; g.ld1 = 256; g.K1 = 256; g.Wp = c->cDb.w; g.bias = c->cDb.b;
  g.M = (capJ + 7) / 8 * nj * 32; g.N = 256; g.cb_total = c->cDb.cbt; g.epi = EPI_STORE_F32; g.out = c->desc; g.ldo = 256;
  g.gr_wgs = c->gemmr_wgs;
  ds.feat = d_junc; ds.n = d_njunc; ds.Bs = nj; ds.B = nj; ds.cap = capJ; ds.HC = R / 8; ds.WC = R / 8;
  ds.w_scale = (float)w / (float)R; ds.h_scale = (float)h / (float)R; ds.flag = nullptr;      // (the junction rows' sample_desc call passes no flag either)
  ds.junc = 1;
}
bool junction_tail_fused(airfe_ctx* c, int nj, int capJ) {
  if (nj < 1 || capJ < 1 || c->prec == 2 || c->cfg.nms_radius != 4 || c->nms_map_valid || c->desc_dense_valid || !c->desc_gather_stream) return false;
  GemmArgs g;
  DescSample ds;
  junction_gemm_args(c, 0, nj, nullptr, capJ, nullptr, 1, 1, g, ds);
  return g.M >= c->gemmr_min && gemmr_gather_sample_junc_applicable(g, ds);
}

// Everything behind the stage-0 tensors for stage slots 0 .. nb-1 (= images i0 .. i0+nb-1 of the detector batch): wireframe_matcher,
// stage 1, the line / junction filter (plnet.cpp:272-307, 468-558) and, for the first nj of them, junction_detector + descriptors
// (plnet.cpp:425-448).  LOI features: the line branch's rows, or (host_s0: the caller's stage-0 tensors were uploaded) the CHW block in c->s0_loi.  Results go to DEVICE buffers:
// d_lines [nb][capL][4], d_nlines / d_lfound [nb], d_junc [nj][capJ][259], d_njunc / d_jfound [nj] (found > cap = the caller's overflow).
// phase: 1 = the lines (needs nothing of the point branch), 2 = the junctions (score maps, descriptor maps of the point branch), 3 = both.
int line_tail_dev(airfe_ctx* c, int i0, int nb, bool host_s0, int h, int w, double* d_lines, int capL, int* d_nlines, int* d_lfound,
                  float* d_junc, int capJ, int* d_njunc, int* d_jfound, int nj, hipStream_t st, int phase) {
  if (!c->has_s1) return fail(c, "PLNet stage-1 weights were not loaded (cfg.plnet_s1_pack)");
  if (nb < 1 || nb > c->Lmax || nj < 0 || nj > nb) return fail(c, "line path: image range outside the arena");
  const bool fused = phase == 3 && junction_tail_fused(c, nj, capJ);
  if (phase & 1) {
    if (!fused) junction_maps_clear(c, nj, st);      // ahead of the dedup, where the clear has always run: the kernel order of the path does not move
    ProfScope ps(c, ST_PL_STAGE1, st, 0, (double)nb * 49152 * 12);
    line_dedup(c, nb, st);
    // host-supplied contract tensors: CHW; else the line branch's head rows (its fused form) or the LOI head at the junctions' tap rows only (its split form)
    const int form = host_s0 ? S1_CHW : c->cfg.line_precision == 3 ? (c->line_sparse ? S1_ROWS_H : S1_HEAD_H) : (c->line_sparse ? S1_ROWS : S1_HEAD);
    if (form == S1_ROWS || form == S1_ROWS_H) {
      if (line_tap_rows(c, nb, st)) return 1;
      line_loi_rows(c, nb, st);
    }
    line_stage1(c, nb, form, 0, st);
  }
  return line_post_dev(c, i0, nb, h, w, d_lines, capL, d_nlines, d_lfound, d_junc, capJ, d_njunc, d_jfound, nj, st, phase, fused);
}

// The byte maps of the first nj images, zeroed for line_filter_maps.  A step of its own: line_tail_dev clears ahead of the dedup, the hooks right before the filter.
void junction_maps_clear(airfe_ctx* c, int nj, hipStream_t st) {
  const int R = AIRFE_INTERNAL_SIZE;
  if (nj > 0) launch_zero16(c->jmap, (size_t)nj * R * R, st);
}

// The line filter over c->s1_la / c->s1_sc / c->wf_counts; the first nj images mark their kept lines' end points in c->jmap (cleared: junction_maps_clear).
void line_filter_maps(airfe_ctx* c, int nb, int nj, int h, int w, double* d_lines, int capL, int* d_nlines, int* d_lfound, hipStream_t st) {
  const int R = AIRFE_INTERNAL_SIZE;
  ProfScope ps(c, ST_PL_FILTER, st, 0, (double)nb * R * R);
  launch_line_filter(c->s1_la, c->s1_sc, c->wf_counts, c->cfg.remove_borders, c->cfg.line_threshold, c->cfg.line_length_threshold, (float)w / (float)R,
                     (float)h / (float)R, R, c->jmap, nj, d_lines, capL, d_nlines, d_lfound, LINE_CAP, nb, st);
}

// junction scores = the NMS'd map at the junction pixels.  Where the dense map was not written (radius 4, large batches) the same values come from
// the raw scores under the NMS's final keep plane: 32 KB per image instead of 1 MB written for < 1024 single-float reads.
struct JunctionScores { bool from_mask; const float* heat; const unsigned long long* mask; };
static JunctionScores junction_scores(airfe_ctx* c, int i0) {
  const int R = AIRFE_INTERNAL_SIZE;
  const bool from_mask = c->cfg.nms_radius > 0 && !c->nms_map_valid;
  return {from_mask, (c->cfg.nms_radius > 0 && !from_mask ? c->heat_nms : c->heat) + (size_t)i0 * R * R,
          from_mask ? reinterpret_cast<const unsigned long long*>(c->nms_mask) + (size_t)i0 * (R / 8) * (R / 8) : nullptr};
}

// junction_detector over c->jmap of the first nj images (= images i0 .. of the detector batch): rows (score, x, y) -> d_junc, descriptor columns untouched.
int junction_scan_maps(airfe_ctx* c, int i0, int nj, float* d_junc, int capJ, int* d_njunc, int* d_jfound, hipStream_t st) {
  const JunctionScores s = junction_scores(c, i0);
  if (s.from_mask && c->cfg.nms_radius != 4) return fail(c, "line path: the NMS'd score maps of this batch were not kept");
  launch_junction_scan(c->jmap, s.heat, AIRFE_INTERNAL_SIZE, c->cfg.remove_borders, d_junc, capJ, d_njunc, d_jfound, c->d_njunc + 2 * c->Lmax, nj, st, s.mask);
  return 0;
}

// The junction rows' descriptors, sampled from the dense descriptor map of images i0 ..
int junction_desc_sample(airfe_ctx* c, int i0, int nj, int h, int w, float* d_junc, int capJ, const int* d_njunc, hipStream_t st) {
  const int R = AIRFE_INTERNAL_SIZE;
  if (!c->desc_dense_valid) return fail(c, "line path: the dense descriptor map of this batch was not made");
  launch_sample_desc(c->desc + (size_t)i0 * (R / 8) * (R / 8) * 256, nj, R / 8, R / 8, d_junc, d_njunc, capJ, (float)w / (float)R, (float)h / (float)R,
                     c->desc_normalised ? 0 : 1, st);
  return 0;
}

// The junction images' dense descriptor maps where the junction tail needs them (plnet_lines_batch, airfe_debug_junction_tail): the point branch of a large batch ran
// the descriptor head on the sampled cells only, so the first nj images' maps are made now (the points have theirs already; c->desc is free to be rewritten) — unless
// the fused tail runs (junction_tail_fused: the head at the junctions' tap rows, no dense map, desc_dense_valid stays false).  partial: only those nj maps exist —
// the caller clears c->desc_dense_valid again once the tail has run.
int junction_dense_maps(airfe_ctx* c, int nj, int capJ, int phase, hipStream_t st, bool& partial) {
  partial = false;
  if (!(phase & 2) || nj < 1 || c->desc_dense_valid || (phase == 3 && junction_tail_fused(c, nj, capJ))) return 0;
  if (dense_desc_head(c, nj, st)) return 1;
  c->desc_dense_valid = true;
  partial = nj != c->last_B;
  return 0;
}

// The end of line_tail_dev: the line filter (phase & 1) and the junction rows of the first nj images (phase & 2).  fused (junction_tail_fused, both phases in one
// call): two launches, no byte maps — else the caller has cleared c->jmap and the dense descriptor map exists.  Shared with the test hook airfe_debug_junction_tail.
int line_post_dev(airfe_ctx* c, int i0, int nb, int h, int w, double* d_lines, int capL, int* d_nlines, int* d_lfound, float* d_junc, int capJ, int* d_njunc,
                  int* d_jfound, int nj, hipStream_t st, int phase, bool fused) {
  const int R = AIRFE_INTERNAL_SIZE;
  if (fused) {
    if (phase != 3 || nj < 1) return fail(c, "line path: the fused junction tail runs both phases in one call");
    {
      const JunctionScores s = junction_scores(c, i0);
      ProfScope ps(c, ST_PL_FILTER, st, 0, (double)nb * LINE_CAP * 20);
      launch_line_filter_junc(c->s1_la, c->s1_sc, c->wf_counts, c->cfg.remove_borders, c->cfg.line_threshold, c->cfg.line_length_threshold, (float)w / (float)R,
                              (float)h / (float)R, d_lines, capL, d_nlines, d_lfound, LINE_CAP, nb, nj, s.heat, s.mask, d_junc, capJ, d_njunc, d_jfound, st);
    }
    GemmArgs g;
    DescSample ds;
    junction_gemm_args(c, i0, nj, d_junc, capJ, d_njunc, h, w, g, ds);
    ProfScope ps(c, ST_HEAD_GEMM, st, 2.0 * g.M * 256 * 256, (double)g.M * 512);
    launch_gemmr_gather_sample_junc(c->prec, g, ds, st);
    return launch_status(c);
  }
  if (phase & 1) line_filter_maps(c, nb, nj, h, w, d_lines, capL, d_nlines, d_lfound, st);
  if ((phase & 2) && nj > 0) {
    ProfScope ps(c, ST_PL_FILTER, st, 0, (double)nj * R * R * 2);
    if (junction_scan_maps(c, i0, nj, d_junc, capJ, d_njunc, d_jfound, st)) return 1;
    if (junction_desc_sample(c, i0, nj, h, w, d_junc, capJ, d_njunc, st)) return 1;
  }
  return launch_status(c);
}

}  // namespace airfe_host
