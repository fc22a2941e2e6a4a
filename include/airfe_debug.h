/* airfe_debug.h — inspection and fault-hunting hooks of libairfe.so.  NOT the drop-in boundary (that is include/airfe.h):
 * nothing on the reference's side binds these; they exist so that tests/ can read internal maps back, feed single kernels
 * with hand-built host tensors, and trace the matcher launch by launch.  Exported by the same library; an integrator may
 * ignore this header entirely. */
#ifndef AIRFE_DEBUG_H_
#define AIRFE_DEBUG_H_
#include "airfe.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- inspection hooks used by the parity tests ------------------------------------------------------ */
/* after a detect call with B images: copy internal maps to HOST buffers (NULL = skip).
 *   heat_raw/heat_nms [B][512][512]; desc [B][64][64][256] (NHWC, channel-normalised). */
int airfe_debug_detector_maps(airfe_ctx* ctx, int B, float* heat_raw, float* heat_nms, float* desc);
/* run LightGlue on one HOST pair (258-float rows) and return the full log-assignment scores [n0][n1] */
int airfe_debug_lightglue_scores(airfe_ctx* ctx, const float* f0, int n0, const float* f1, int n1, float* scores);
/* the post-processing kernels alone on HOST score matrices (hand-built ties, -inf rows, threshold-exact values):
 *   filter_matches (src/light_glue.cpp:214-266) on scores [n0][n1]; decode (src/super_glue.cpp:339-367) on Z [n0+1][n1+1] */
int airfe_debug_lg_filter(airfe_ctx* ctx, const float* scores, int n0, int n1, int32_t* idx, float* score, int cap, int* nmatch);
int airfe_debug_sg_decode(airfe_ctx* ctx, const float* Z, int n0, int n1, int32_t* idx0, int32_t* idx1, double* ms0, double* ms1);
/* the Sinkhorn launcher alone (launch_sg_sinkhorn: the optimal-transport tail of SuperGlue) on B HOST coupling matrices, one form at a time
 * (tests/test_gpu_sinkhorn.py).  Pair b's couplings sim[b][0..n0)[0..n1) go into the matcher's similarity buffer at its own stride; the REST of every pair's block,
 * the output buffer and the partial-exchange buffer are NaN when the launch starts, so a finite Z proves that no form read outside `lens` and that every
 * element was written.  alpha (the dustbin score) and iters come from the call, not from the context.  form: 0 = the launcher's own dispatch (what production
 * runs), 1 = the per-half-iteration kernels, 2 = the register-resident cooperative kernel — an ERROR where no instantiation applies or the cooperative launch is
 * refused, never a fall-back.  *form_ran: 1 = per-half-iteration, 2 = sg_sinkhorn_reg_kernel<13, 7>, 3 = sg_sinkhorn_reg_kernel<9, 17>.  B <= max_batch,
 * 1 <= n0, n1 <= min(ld, max_keypoints).  Z[b] holds rows 0..n0, cols 0..n1 (row stride ld + 1); the rest of Z is not touched.  Reports a rendezvous
 * time-out like the host entries do. */
int airfe_debug_sg_sinkhorn(airfe_ctx* ctx, const float* sim, const int* lens /*[2B]: n0,n1 per pair*/, int B, int ld /*row stride and rows per pair of sim*/,
                            float alpha, int iters, int form /*0 auto, 1 per-half-iteration, 2 register-resident*/, float* Z /*[B][ld+1][ld+1]*/, int* form_ran);
/* kernel-level checks on HOST fp32 tensors (test only): NCHW conv3x3(+ReLU, optional 2x2 max-pool) and
 *   y[M][N] = x[M][K] w[N][K]^T + b through the same MFMA kernels the pipelines use. */
/* SuperGlue on one HOST pair ([n][259] rows, normalised x,y): the engine's `scores` output [n0+1][n1+1] */
int airfe_debug_superglue_scores(airfe_ctx* ctx, const float* f0, int n0, const float* f1, int n1, float* scores);
/* the on-device stage-0 line branch of the last detected image in the Appendix A.1 layouts + the junction probability / offset
 *   maps behind juncs_pred (any pointer may be NULL): juncs_pred [300][2], lines_pred [49152][4], iskeep / idx_min / idx_max [49152],
 *   loi [128][128][128], thin / aux [4][128][128], jloc [128][128], joff [2][128][128] */
int airfe_debug_plnet_stage0(airfe_ctx* ctx, float* juncs_pred, float* lines_pred, float* iskeep, float* idx_min, float* idx_max,
                             float* loi, float* thin, float* aux, float* jloc, float* joff);
/* the junction-to-line match (HAWP wireframe_matcher) of the LAST detected image: fast = 1 as the line path runs it (cell search: iskeep
 * exact everywhere, idx_junc_to_end_min / _max exact where iskeep > 0 — all that src/plnet.cpp:272-307 reads), fast = 0 the contract's
 * tensors in full.  [3*128*128] floats each, NULL = skip. */
int airfe_debug_plnet_j2l(airfe_ctx* ctx, int fast, float* iskeep, float* idx_min, float* idx_max);
/* wireframe_matcher + stage-1 LOI head alone: lines_adjusted [cap][4], scores_line [cap], *m2 = unique lines */
int airfe_debug_plnet_s1(airfe_ctx* ctx, const airfe_plnet_stage0* stage0, float* lines_adjusted, float* scores_line,
                         int cap, int* m2);
/* the stage-1 outputs of image 0 of the LAST PLNet call as the line path left them on the device (the device path's own kernel: cfg.line_precision decides which):
 * lines_adjusted [cap][4], scores_line [cap], *m2 = unique candidate lines */
int airfe_debug_plnet_s1_last(airfe_ctx* ctx, float* lines_adjusted, float* scores_line, int cap, int* m2);
/* the pre-process alone (cv::resize + /255, src/plnet.cpp:246-270): HOST gray image -> HOST fp32 [512][512] */
int airfe_debug_preprocess(airfe_ctx* ctx, const uint8_t* gray, int h, int w, int stride, float* out);
int airfe_debug_conv3x3(airfe_ctx* ctx, const float* x, int B, int cin, int H, int W, const float* w, const float* b,
                        int cout, int pool, float* y);
int airfe_debug_gemm(airfe_ctx* ctx, const float* x, int M, int K, const float* w, const float* b, int N, int relu, float* y);
/* ---- the encoder's 3x3 convolutions one launch at a time, every form the arena runs (tests/test_gpu_conv_kernels.py, tests/conv_ref.py).  HOST fp32 tensors in,
 * rounded to the context's 2-byte type on the way in; the WHOLE device output buffer back as 2-byte words, so that the caller sees what the launch wrote and what it
 * left alone.  Nothing here has a kernel of its own.
 *   plain form (x given): launch_conv3x3, i.e. production's dispatch — conv64r_kernel (cin 64) / conv128r_kernel (cin 128) with relu = 1, conv3x3_kernel with relu = 0.
 *   fused form (img given): launch_conv64r with ConvArgs::img set, as the detector launches conv1a -> conv1b -> 2x2 max-pool.  img [B][H][W] is staged as fp32
 *     [B][H+2][W+2] with a zero border; w1a / b1a go to the device as fp32.  The kernel's contract: image, w1a and b1a are converted to fp16 in BOTH storage modes (conv1a
 *     runs on the fp16 MFMA), conv1a's output is stored in the storage type, and it is exactly 0 at halo pixels outside the image.
 * y_raw holds guard | buffer | guard: the buffer is [B][Ho + 2 out_pad][Wo + 2 out_pad][cout] (Ho, Wo = H, W halved by pool), a guard is one buffer row,
 * (Wo + 2 out_pad) cout words; y_words = the three together.  Every byte of all three is 0xFF when the launch starts (0xFFFF is a NaN in both types).
 * wgs = ConvArgs::wgs, the persistent kernels' workgroup cap (256 = production's grid; lower, and a small input wraps the tile loop).  conv3x3_kernel ignores it.
 * Refused before any launch, with the context left usable: wgs outside 1 .. 256; cin other than 64 / 128; cout no multiple of 64 (of 128 when cin = 128); H or W no
 * multiple of 16; pool with out_pad = 0 (every pooled layer of the arena feeds another conv, so that form exists nowhere and stays untested); the fused form with
 * anything but cin = cout = 64, pool = 1, out_pad = 1, relu = 1; both or neither of x and img; a y_words that is not the size above. */
typedef struct airfe_debug_conv_args {
  const float* x;                 /* [B][cin][H][W], or NULL: the fused form */
  const float* img;               /* [B][H][W] (the fused form), or NULL */
  const float *w1a, *b1a;         /* [64][9], [64] (the fused form) */
  const float *w, *b;             /* [cout][cin][3][3], [cout] */
  int cin, cout, B, H, W;
  int pool, out_pad, relu, wgs;
  size_t y_words;
  uint16_t* y_raw;                /* [y_words] out */
} airfe_debug_conv_args;
int airfe_debug_conv(airfe_ctx* ctx, airfe_debug_conv_args* a);
/* Tile order of conv64r_kernel (bit 0) and conv128r_kernel (bit 1), process-wide and read once per launch (csrc/conv_tile_order.h): bit set = workgroups placed by
 * XCD over 2-D blocks of tiles with a layer's cout passes in one launch, bit clear = raster order, one launch per pass.  The per-tile arithmetic is the same: every
 * output byte is (tests/test_gpu_conv_tile_order.py).  order 0 .. 3 sets it, -1 restores the library's default; *previous (may be NULL) receives the value before
 * the call.  For A/B measurements (bench.py --tuning conv_order=0) and that test; not for use beside running work. */
int airfe_debug_conv_order(int order, int* previous);
/* ---- the matcher's / detector's GEMM family one form at a time (tests/test_gpu_linear_kernels.py, tests/test_gpu_lg_block.py).  HOST fp32 tensors in, rounded to the
 * 2-byte type `prec` (0 = bf16, 1 = fp16) on the way in; weights packed as the pipelines pack them (scale 1); HOST fp32 out in the kernel's own layout.  The kernels
 * are the production ones: nothing here has a kernel of its own. */
enum {
  AIRFE_DEBUG_KERNEL_DISPATCH = 0,        /* launch_gemm's own choice by the context's row thresholds (EPI_SOFTMAX_D2S: launch_gemm8's head kernel) */
  AIRFE_DEBUG_KERNEL_SMALL = 1,           /* gemm_small_kernel */
  AIRFE_DEBUG_KERNEL_TILED = 2,           /* gemm_kernel */
  AIRFE_DEBUG_KERNEL_GEMM8 = 3,           /* gemm8_kernel (head_softmax_d2s_kernel for EPI_SOFTMAX_D2S) */
  AIRFE_DEBUG_KERNEL_GEMMR = 4,           /* gemmr_kernel */
  AIRFE_DEBUG_KERNEL_GEMMR_GATHER = 5,    /* gemmr_gather_kernel */
  AIRFE_DEBUG_KERNEL_GEMMR_GATHER128 = 6  /* gemmr_gather128_kernel */
};
/* One linear y = W cat(x1, x2) + b through epilogue `epi` (airfe::Epi: 0 store, 1 store fp32, 2 residual, 3 heads, 4 heads transposed, 5 soft-max + depth-to-space).
 * The rows are padded with zero rows to the forced kernel's row tile (DISPATCH: 128, as the matcher pads its token count); only the first M come back.  A forced
 * kernel that does not apply to the form is an ERROR, never a fall-back to another kernel. */
typedef struct airfe_debug_linear_args {
  int prec, M, K, K1, N;          /* K in {128, 256, 512}; K1 = K without x2 */
  const float* x1;                /* [M][K1] ([src_rows][K1] with rowidx) */
  const float* x2;                /* [M][K - K1] or NULL */
  const float* w;                 /* [N][K] */
  const float* b;                 /* [N] */
  int epi, act;                   /* act: 1 = ReLU */
  const int* rowidx;              /* [M] source rows of x1 (gather) or NULL */
  int src_rows;
  const float* rot_cos;           /* [M][32] (EPI_HEADS rotary) or NULL */
  const float* rot_sin;
  int Np, H;                      /* head layouts: M = S * Np, H heads of 64 */
  float* x32;                     /* EPI_RESID: [M][N] residual in, x32 + W x + b out */
  int d2s_hc, d2s_wc;             /* EPI_SOFTMAX_D2S: M = B * hc * wc cells, N = 65 */
  int* flag;                      /* EPI_SOFTMAX_D2S: 1 when a cell's logits were not finite */
  int kernel;                     /* AIRFE_DEBUG_KERNEL_* */
  int gr_wgs;                     /* streaming kernels' workgroups (<= 0: the context's) */
  float* out;                     /* [M][N] | heads [S][H][Np][64] (N = 512: q) | transposed [S][H][64][Np] | heat [B][8 hc][8 wc] */
  float* out2;                    /* EPI_HEADS with N = 512: k [S][H][Np][64] */
} airfe_debug_linear_args;
int airfe_debug_linear(airfe_ctx* ctx, const airfe_debug_linear_args* a);
/* one layer's attention inputs over rows x [M][256]: head-major q|k (wqk [nqk][256], nqk = 512 with rotary (q -> q, k -> k) or 256 (-> q)) and transposed V
 * (wv [256][256] -> vt [S][4][64][Np]); pair = 1: ONE gemmr_pair launch (an error where it does not apply), 0: the two linears through launch_gemm's dispatch */
int airfe_debug_qkv(airfe_ctx* ctx, int prec, int M, int Np, const float* x, const float* wqk, const float* bqk, int nqk, const float* wv, const float* bv,
                    const float* rot_cos, const float* rot_sin, int pair, int gr_wgs, float* q, float* k, float* vt);
/* the fused post-attention block (launch_lg_blockf) on HOST tensors.  xb is built as the 2-byte copy of x32 (the pipeline's invariant).  Every buffer has
 * rows_cap >= M + 256 rows (input rows past M are zero); output rows past M start as a canary, and rows_past[0..4] = rows past M that the launch wrote in
 * x32, xb, q, k, vt (0: none). */
typedef struct airfe_debug_lg_block_args {
  int prec, M;
  const float* attn;              /* [M][256] */
  float* x32;                     /* [M][256] in / out */
  float* xb;                      /* [M][256] out */
  const float *wo, *bo;           /* [256][256], [256]; NULL: w1's message half is already folded (the kernel's ffn.0 reads cat(x, attn)) */
  const float *w1, *b1;           /* [512][512], [512] */
  const float *gamma, *beta;      /* [512] */
  const float *w2, *b2;           /* [256][512], [256] */
  int relu;                       /* 1: ReLU instead of LayerNorm + GELU */
  int tokens_per_wg, mixed;       /* 32, 64, 112, 128; mixed: the two-round split (folded, 112) on the device's CUs */
  int nqk_n;                      /* 0: no next projection; 512: q | k with rotary; 256: shared */
  const float *nqk_w, *nqk_b;     /* [nqk_n][256], [nqk_n] */
  const float *nv_w, *nv_b;       /* [256][256], [256] */
  const float *rot_cos, *rot_sin; /* [M][32] (nqk_n = 512) */
  int Np;                         /* head layouts: M = S * Np */
  float *q, *k, *vt;              /* [S][4][Np][64] x 2, [S][4][64][Np] */
  int rows_past[5];
} airfe_debug_lg_block_args;
int airfe_debug_lg_block(airfe_ctx* ctx, airfe_debug_lg_block_args* a);
/* launch_ln_gelu in place on h [M][512] (rounded to the 2-byte type on the way in) */
int airfe_debug_ln_gelu(airfe_ctx* ctx, int prec, float* h, const float* gamma, const float* beta, int M);
/* the matcher's flash attention alone (kernels_attn.hip) on HOST fp32 tensors, rounded to the matcher's 2-byte type on the way in: q, k [S][H][n][64] with the
 * soft-max scale and log2 e ALREADY inside (the kernel computes p = 2^(q.k - shift)), v [S][H][n][64], lens [S] (keys / queries beyond lens[s] are padding), cross:
 * sequence s attends to sequence s ^ 1.  out [S][n][H*64] fp32.  n <= max_keypoints (rounded up to 16 inside); S * H a multiple of 8.  The way to drive the kernel's
 * re-centring path (a tile whose partial row sums leave the 2-byte range) with hand-built logits. */
int airfe_debug_attention(airfe_ctx* ctx, const float* q, const float* k, const float* v, const int* lens, int S, int H, int n, int cross, float* out);
/* the same launch with the 2-byte type per call (one context serves both instantiations) and, with canary = 1, an output buffer that is 0xFF bytes (NaN in both
 * types), its 128 slack rows included, when the launch starts: the rows come back as the device left them, so a finite row is one that THIS launch wrote, and
 * rows_past counts the slack rows behind the last sequence that it changed (0: none).  The K, Q and V^T slack behind the last sequence stays zero, as the arena's is:
 * V^T is read there under a zero weight, and 0 * NaN would be NaN.  raw = 1: all Np = 16 ceil(n / 16) rows of every sequence come back (out [S][Np][H*64]) instead of
 * the first n.  lens[s] = 0 is allowed on either side.  airfe_debug_attention is this entry with the context's matcher_precision, canary = 0 and raw = 0.  Nothing
 * here has a kernel of its own, and no production launch path changes. */
typedef struct airfe_debug_attn_args {
  int prec;                       /* 0 = bf16, 1 = fp16 */
  int S, H, n, cross;             /* S * H a multiple of 8; cross: S even */
  const float *q, *k, *v;         /* [S][H][n][64] */
  const int* lens;                /* [S], each 0 .. n */
  int canary, raw;
  float* out;                     /* [S][raw ? Np : n][H*64] */
  int Np, rows_past;              /* out */
} airfe_debug_attn_args;
int airfe_debug_attention_args(airfe_ctx* ctx, airfe_debug_attn_args* a);
/* ---- LightGlue's head and tail one launcher at a time (tests/test_gpu_lg_tail.py, tests/lg_tail_ref.py).  HOST tensors in, the production launchers on the
 * context's own arena, HOST tensors out; nothing here has a kernel of its own, and no production launch path changes. */
/* launch_lg_prepare alone.  EVERY token row of the arena (x32, xb, rot_cos, rot_sin, the slack included) is 0xFF bytes (NaN in every type) when the launch
 * starts, so a finite output row was written by this launch; rows_past counts the arena rows at or beyond `rows` that the launch changed (0: none).  The arena is
 * zero again when the hook returns.  Bt = B, or 2 with the second pair (f0x: B must be 1); rows = 2 Bt Np + slack_rows <= the arena's rows. */
typedef struct airfe_debug_lg_prepare_args {
  int prec;                       /* 0 = bf16, 1 = fp16 (the type of xb) */
  int B, cap, ld, kp_off;         /* f0 / f1 [B][cap][ld] rows, x at column kp_off, the 256 descriptor floats from kp_off + 2 (ld 259: kp_off 1; ld 258: 0) */
  int normalize;
  float cx, cy, linv;
  const float *f0, *f1;
  const int *n0, *n1;             /* [B], each 0 .. cap */
  const float* wr;                /* [32][2] */
  const float *f0x, *f1x;         /* the second pair's rows [n0x][ld], [n1x][ld], or both NULL */
  int n0x, n1x;
  int slack_rows;
  int rows;                       /* 2 Bt Np + slack_rows: the rows of the four outputs */
  float *x32, *xb;                /* [rows][256]; xb widened to float */
  float *rot_cos, *rot_sin;       /* [rows][32] */
  int* lens;                      /* [2 Bt] */
  int rows_past;
} airfe_debug_lg_prepare_args;
int airfe_debug_lg_prepare(airfe_ctx* ctx, airfe_debug_lg_prepare_args* a);
/* launch_rowdot256, then form 0: launch_sim + launch_lg_assign (lg_lse_kernel / lg_arg_kernel for B <= 8, the four separate kernels above) or form 1:
 * launch_lg_assign_fused with sim_out and scores_out set.  Sequence s (0 .. 2B-1; pair b = sequences 2b, 2b + 1) has lens[s] rows (0 allowed) of md and x32, n rows
 * apart.  When the launches start: rows of mdb and x32 at or beyond a sequence's length are 0xFF bytes (NaN) — or, with `pad` [256] given, mdb's hold `pad` rounded to
 * `prec` (a finite value that an unmasked maximum would pick up, which a NaN is not: fmaxf drops it); simbuf, both partial arrays, rowlse, collse, scores,
 * rowval and score are NaN, nmatch is 0xFF, and rowarg, colarg and idx are ZERO — the value that passes for a valid index.  Outputs are dense per pair with stride
 * n (cap for idx / score) and come back as the device left them, poison included, over all n rows and columns. */
typedef struct airfe_debug_lg_assign_args {
  int prec, B, n;                 /* n <= Np */
  const float* md;                /* [2B][n][256], rounded to prec by the hook */
  const float* x32;               /* [2B][n][256] */
  const float* w;                 /* [256] matchability weight */
  float b;
  const int* lens;                /* [2B] */
  int cap;                        /* 1 .. Np */
  float thr;
  int form;
  const float* pad;               /* [256] or NULL */
  float* z;                       /* [2B][n] */
  float *sim, *scores;            /* [B][n][n] */
  float *rowlse, *collse, *rowval;/* [B][n] */
  int32_t *rowarg, *colarg;       /* [B][n] */
  int32_t* idx;                   /* [B][cap][2] */
  float* score;                   /* [B][cap] */
  int32_t* nmatch;                /* [B] */
} airfe_debug_lg_assign_args;
int airfe_debug_lg_assign(airfe_ctx* ctx, airfe_debug_lg_assign_args* a);
/* SuperGlue's front alone (sg_front_dev, the statement superglue_dev runs: the slack-row reset, launch_sg_prepare and, split, the two memsets of the surplus rows and
 * the two GEMMs of the keypoint encoder's large layers) on HOST feature rows (tests/test_gpu_sg_front.py, tests/sg_front_ref.py).  The normalisation constants are the
 * context's own (cfg.image_width / image_height, scale 0.7).  EVERY row of x32, xb, msg and hb in the arena, and lens, is 0xFF bytes (NaN in every type) when the launches
 * start, so a finite output was written by this call.  prec names the context's 2-byte type (matcher_precision) and is refused when it differs; under a fp32 context
 * (matcher_precision 2) only the unsplit form exists and prec is 1, the fp16 shadow production asks for.  M = 2 B Np, rows = Mg = M rounded up to 128: the rows the
 * GEMMs run over.  rows_past counts the arena rows at or beyond `rows` whose x32 or xb bytes are neither zero (what the slack-row reset leaves) nor the fill.  The
 * arena is zero again when the hook returns. */
typedef struct airfe_debug_sg_front_args {
  int prec, split;                /* prec 0 = bf16, 1 = fp16; split 1 = the large layers as GEMMs */
  int B, cap, normalize;          /* f0 / f1 [B][cap][259] rows (score, x, y, descriptor), 1 <= cap <= Np */
  const float *f0, *f1;
  const int *n0, *n1;             /* [B], each 0 .. cap */
  int rows;                       /* Mg */
  int* lens;                      /* [2 B] */
  float *x32, *xb;                /* [rows][256]; xb widened to float */
  float *h128, *hb;               /* split: [rows][128], [rows][256], widened; unused (may be NULL) otherwise */
  int rows_past;
} airfe_debug_sg_front_args;
int airfe_debug_sg_front(airfe_ctx* ctx, airfe_debug_sg_front_args* a);
/* ---- the index work behind the networks on hand-built maps (tests/test_gpu_detector_tail_pin.py, tests/detector_tail_ref.py): exact ties, plateaus, exact zeros, scores
 * equal to the threshold, peaks on the border lines — inputs the soft-max maps of real images never hold.  HOST tensors are staged into the context's own buffers and the
 * launchers production calls run in production's order with production's arguments; nothing here has a kernel of its own.  Each reports an activation-range overflow as the
 * host entries do. */
/* Everything airfe's detector runs behind the score head (detect_tail_dev, the function detect_dev2 ends in): NMS by cfg.nms_radius, candidate compaction, top-K
 * (cfg.max_keypoints, cfg.keypoint_threshold, cfg.remove_borders), the descriptor head and descriptor sampling.  The forms are chosen as production chooses them: by B, cap and
 * the context's tuning (B <= 2: dense NMS'd map, dense head, sample_desc; B > 2 and cap <= 1024: no dense map, the head as a gather GEMM over the sampled cells — tiled, or
 * streaming with the sampling inside from airfe_tuning::gemmr_min_m rows on).  heat: finite, in [0, 1].  act: the convDa activations, rounded to the context's 2-byte type on
 * the way in.  Bs = 0: one destination (feat / n, B images); else B = 2 Bs and images b >= Bs go to feat1 / n1, as in a stereo call.  feat / feat1 / n / n1 are uploaded as the
 * caller filled them and come back whole, so a sentinel shows every write to a row k >= n[b].  nms_map comes back only where the form wrote it (nms_map_written = 1; the buffer is
 * left alone otherwise); keep = the final keep plane (radius 4 only; word [image][band][lane], byte = row 8 band + r, bit = column 8 lane + j). */
typedef struct airfe_debug_detector_tail_args {
  int B, Bs, h, w, cap;           /* h, w: the image size the keypoints are scaled to */
  const float* heat;              /* [B][512][512] */
  const float* act;               /* [B][64][64][256] */
  float *feat, *feat1;            /* [B or Bs][cap][259], [B - Bs][cap][259] or NULL; in / out */
  int *n, *n1;                    /* [B or Bs], [B - Bs] or NULL; in / out */
  float* nms_map;                 /* [B][512][512] or NULL */
  unsigned long long* keep;       /* [B][64][64] or NULL */
  int* cand_cnt;                  /* [B] or NULL */
  int nms_map_written;            /* out */
} airfe_debug_detector_tail_args;
int airfe_debug_detector_tail(airfe_ctx* ctx, airfe_debug_detector_tail_args* a);
/* The line path's filter and junction scan (line_tail_dev's launch_zero16, launch_line_filter, launch_junction_scan; no descriptor sampling) on hand-built stage-1 outputs:
 * la [B][ld][4] / sc [B][ld] with m2[b] <= ld lines each go to the stage-1 buffers, heat to the score maps.  The point branch's radius-4 NMS runs first, from_plane = 0 with the
 * dense NMS'd map (the junction scan reads it), 1 without (the scan reads raw scores under the keep plane).  lines / junc are uploaded as the caller filled them and come
 * back whole: columns 3 .. 258 of every junction row and all rows past the counts keep the caller's sentinel.  nfound / jfound: the true counts (> cap = the overflow).
 * jmap (optional): junction maps [nj][512][512] bytes that replace the filter's between the two launches — the filter marks no pixel outside the scan's box, so the scan's
 * own bounds show only on a map that has such pixels. */
typedef struct airfe_debug_line_post_args {
  int B, nj, ld, h, w, capL, capJ, from_plane;
  const float *la, *sc;           /* [B][ld][4], [B][ld] */
  const int* m2;                  /* [B] */
  const float* heat;              /* [B][512][512] */
  double* lines;                  /* [B][capL][4] in / out */
  int *nlines, *nfound;           /* [B] out */
  float* junc;                    /* [nj][capJ][259] in / out */
  int *njunc, *jfound;            /* [nj] out */
  const unsigned char* jmap;      /* [nj][512][512] or NULL */
} airfe_debug_line_post_args;
int airfe_debug_line_post(airfe_ctx* ctx, airfe_debug_line_post_args* a);
/* The junction tail of the batched line path, line filter -> junction descriptors, in the form production chooses (line_post_dev, the function line_tail_dev ends in): with
 * the dense maps gone (B > 2: radius-4 keep plane, no dense descriptor map) and the streaming gather GEMM applicable at ceil(capJ / 8) * nj * 32 rows (>=
 * airfe_tuning::gemmr_min_m) the junction list is built inside the line filter from a bitmap in LDS and the descriptors come from the sampling gather GEMM at the junctions'
 * tap rows (fused = 1); else the byte maps, the two scan launches, the dense descriptor head (of all B <= 2 images, as the detector leaves it, or of the nj junction images)
 * and sample_desc run (fused = 0).  la / sc / m2 / heat as airfe_debug_line_post takes them; act: convDa activations, rounded to the context's 2-byte type on the way in.
 * lines / junc are uploaded as the caller filled them and come back whole: rows past the counts keep the caller's sentinel, rows below them hold score, x, y (scaled to
 * w, h) and the 256 descriptor columns.  nfound / jfound: the true counts (> cap = the overflow). */
typedef struct airfe_debug_junction_tail_args {
  int B, nj, ld, h, w, capL, capJ;
  const float *la, *sc;           /* [B][ld][4], [B][ld] */
  const int* m2;                  /* [B] */
  const float* heat;              /* [B][512][512] */
  const float* act;               /* [B][64][64][256] */
  double* lines;                  /* [B][capL][4] in / out */
  int *nlines, *nfound;           /* [B] out */
  float* junc;                    /* [nj][capJ][259] in / out */
  int *njunc, *jfound;            /* [nj] out */
  int fused;                      /* out */
} airfe_debug_junction_tail_args;
int airfe_debug_junction_tail(airfe_ctx* ctx, airfe_debug_junction_tail_args* a);
/* get_junctions alone (junctions_topk_dev, the function the line branch calls): jloc [B][128][128], joff [B][2][128][128] -> juncs_pred [B][300][2] (rows past the number of
 * positive 3x3 maxima: 0, 0) */
int airfe_debug_junctions_topk(airfe_ctx* ctx, const float* jloc, const float* joff, int B, float* juncs_pred);
/* ---- the line path between the stage-0 tensors and the line filter, one launcher at a time (tests/test_gpu_line_mid_pin.py, tests/line_mid_ref.py): the junction-to-line
 * match (launch_s0_j2l), the kept list and the unique pairs (launch_wireframe), the junctions' tap rows and projections (launch_s1_junc_rows, launch_s1_junc_proj,
 * launch_s1h_junc_proj) and stage 1 (launch_plnet_s1, launch_plnet_s1h) on hand-built HOST tensors: exact ties, threshold-exact distances, junctions on cell borders, (0, 0)
 * padding junctions, more than 8192 kept proposals (wireframe_kernel's long path), more line tiles than workgroups (the stage-1 kernels' tile hand-over).  The tensors are
 * staged into the context's own line-path buffers and the launchers production calls run in production's order with production's arguments (line_branch_dev / line_tail_dev);
 * nothing here has a kernel of its own.  B <= the arena's images.
 *   j2l: 0 = iskeep_in / idx_min_in / idx_max_in are staged as given (launch_wireframe counts the kept proposals itself: counted = false); 1 = launch_s0_j2l's brute-force
 *     kernel (exact_all = 1); 2 = the line path's call (exact_all = 0, the cell search) with `counts` passed, its return value going to launch_wireframe as `counted`.
 *   s1_form: 0 = launch_plnet_s1 on the contract's CHW tensors (loi transposed on the host; B = 1); 1 = launch_s1_junc_proj from head rows (loi staged at pitch 160, B = 1) +
 *     plnet_s1_kernel<true>; 2 = launch_s1_junc_rows, tap rows, launch_s1_junc_proj(lrows), plnet_s1_kernel<true>; 3 = launch_s1_junc_rows, tap rows,
 *     launch_s1h_junc_proj, launch_plnet_s1h.  Forms 2 and 3: the hook reads ridx back and gathers the four tap rows of every junction from the host loi ON THE HOST (the
 *     gather GEMM is pinned by tests/test_gpu_linear_kernels.py), every index checked against the image's 16384 rows first.
 *   wgs: workgroups per image of the stage-1 launch (0 = production's rule by B; lower, and a workgroup walks several 32-line tiles).
 * EVERY output buffer is 0xFF bytes when the launches start (iskeep / idx_min / idx_max only where the device computes them), and all of it comes back as the device left
 * it, capacity rows included: a finite or valid entry was written by this run.  head4 is read back between launch_wireframe and stage 1, and the buffer — production's
 * lines_adjusted — is 0xFF again before forms 0 .. 2 run (their kernel writes lines_adjusted itself; form 3 reads what launch_wireframe left).  table_dirty[b] = entries of
 * image b's pair table that are not 0x7FFFFFFF after the run (wireframe_kernel promises to leave it clean; the hook does not repair it).
 * Refused before any launch, the context left usable: B outside the arena; forms 0 and 1 with B > 1; j2l = 0 without the three index tensors; wgs outside 0 .. 512; form 3
 * without the split weights; a j2l or s1_form outside the lists above; a junction or proposal coordinate that is not finite.
 * LINE_CAP (45056) exceeds the 44850 pairs 300 junctions can form and KEEP_CAP equals the proposal count, so the launchers' overflow branches (pos >= cap, pos >= line_cap,
 * min(m1, cap)) cannot be reached through production's arguments and stay untested. */
typedef struct airfe_debug_line_mid_args {
  int B, j2l, s1_form, wgs;
  const float* juncs_pred;                            /* [B][300][2] */
  const float* lines_pred;                            /* [B][49152][4] */
  const float *thin, *aux;                            /* [B][4][128][128]: staged as the CHW planes and as the pixel-major thin | aux copy */
  const float* loi;                                   /* [B][128*128][128] pixel-major */
  const float *iskeep_in, *idx_min_in, *idx_max_in;   /* [B][49152] (j2l = 0) or NULL */
  float *iskeep, *idx_min, *idx_max;                  /* [B][49152] out */
  int32_t* counts;                                    /* [B][2] out: M1, M2 */
  int32_t* keep;                                      /* [B][49152] out */
  int32_t *pairs, *rep;                               /* [B][45056][2], [B][45056] out */
  float *head4, *prop4;                               /* [B][45056][4] out */
  int32_t* ridx;                                      /* [B][300][4] out (forms 2, 3; else left alone) */
  float* proj;                                        /* [B][300][256] out (forms 1 .. 3; else left alone) */
  float *lines_adjusted, *scores_line;                /* [B][45056][4], [B][45056] out */
  int32_t* table_dirty;                               /* [B] out */
} airfe_debug_line_mid_args;
int airfe_debug_line_mid(airfe_ctx* ctx, airfe_debug_line_mid_args* a);
/* ---- the stage-0 decode between the line head and the stage-0 tensors (kernels_s0.hip; tests/test_gpu_s0_decode_pin.py, tests/s0_decode_ref.py): s0_decode_kernel with
 * s0_jnms_kernel and s0_loi_chw_kernel (launch_s0_decode), s0_head_decode_kernel (launch_s0_head_decode) and the two-pass form behind airfe_tuning::fuse_dec = 0, on hand-built
 * HOST head rows or line features.  The input is staged into the context's own buffers and the launcher production calls runs with production's arguments (line_branch_dev);
 * nothing here has a kernel of its own.
 *   mode 0, rows: head rows [B][128*128][ld] with the 17 decoded channels (md0..2 dis res | jloc0 jloc1 | joffx joffy | thin0..3 | aux0..3) from column off, one of
 *     production's two layouts (ld 160, off 128: the fused 145-channel head, staged in l_head — which holds one image, so B > 1 uses a buffer of the call; ld 32, off 0: the
 *     17-channel head, staged in l_dec).  launch_s0_decode with ta8 / loi / jnms passed or NULL by want_ta8 / want_loi (ld 160 only: the CHW copy of image 0's columns
 *     0 .. 127) / want_jnms.
 *   mode 1, features: x [B*128*128][128] line features, rounded to the 2-byte type prec (0 = bf16, 1 = fp16) on the way in and staged in l_feat; head weight w [17][128] and
 *     bias b [17], packed by make_linear as airfe_debug_linear packs.  launch_s0_head_decode(wgs): lines_pred, jloc, joff, the pixel-major thin | aux; want_jnms.
 *   mode 2, features, two passes: the same input through launch_gemm (small_max = 1 << 30, EPI_STORE_F32, ldo 32) into l_dec, then launch_s0_decode(32, 0) with ta8 and the
 *     CHW planes, as line_branch_dev runs it with fuse_dec = 0.  head_rows: l_dec as the GEMM left it.
 * EVERY output buffer is 0xFF bytes when the launches start — the stage blocks of all B slots whole, jloc, joff, jnms, ta8, the CHW loi buffer, l_dec in mode 2 — and all of
 * it comes back as the device left it: stage [B][stage_floats] holds juncs_pred | lines_pred | iskeep | min | max | thin | aux at the offsets of airfe_host.h (SG_*), so
 * poison shows where the contract writes nothing.  jnms has no buffer in the context (the line path takes the candidates inside launch_candidates_nms3): a buffer of the call.
 * Refused before any launch, the context left usable: B outside the arena; a mode outside 0 .. 2; a layout other than the two above; want_loi without ld 160; prec outside
 * 0 / 1; wgs outside 0 .. 4096; a stage_floats that is not the library's stage stride; a missing pointer. */
typedef struct airfe_debug_s0_decode_args {
  int B, mode;
  int ld, off;                    /* mode 0 */
  int want_ta8, want_loi, want_jnms;
  int prec, wgs;                  /* modes 1, 2 (wgs: mode 1) */
  const float* rows;              /* [B][128*128][ld] (mode 0) */
  const float* x;                 /* [B*128*128][128] (modes 1, 2) */
  const float *w, *b;             /* [17][128], [17] (modes 1, 2) */
  size_t stage_floats;            /* floats per stage block: must equal the library's stride */
  float* stage;                   /* [B][stage_floats] out */
  float *jloc, *joff, *jnms;      /* [B][128*128], [B][2][128*128], [B][128*128] out */
  float* ta8;                     /* [B][128*128][8] out */
  float* loi;                     /* [128][128*128] out: the context's one-image CHW buffer */
  float* head_rows;               /* [B][128*128][32] out (mode 2; else left alone) */
} airfe_debug_s0_decode_args;
int airfe_debug_s0_decode(airfe_ctx* ctx, airfe_debug_s0_decode_args* a);
/* error-path test of cfg.check_launches: the NEXT group of launches of profiling stage `stage` (airfe_profile_stage_name's index) is preceded by one
 * deliberately invalid launch (4096 threads per workgroup), so that the entry that makes it must fail with "<stage name>: kernel launch failed: ..." —
 * with check_launches = 0 the same failure surfaces at the pipeline's end without the stage.  -1 disarms. */
int airfe_debug_fail_next_launch(airfe_ctx* ctx, int stage);
/* fault hunting (tools/experiments/matcher_trace.py): position-dependent 64-bit checksums of the LightGlue forward's state behind EVERY launch
 * (src/light_glue.cpp:120-170 is one opaque engine call; here it is ~60 launches) — residual stream, token shadow, q / k / v^T, attention
 * output, descriptors, similarity, assignment vectors — in units of 16 token rows (v^T: one feature row).  airfe_debug_trace(ctx, 1) switches it on
 * for the following matcher calls (+~2 ms per 64-pair step); _slots / _slot describe the slots of the last call (name, first unit, units,
 * 32-bit words per unit); _read synchronises `stream` (NULL: the context's) and copies one digest per slot and / or the whole unit table. */
int airfe_debug_trace(airfe_ctx* ctx, int on);
/* slot >= 0: the forward pass returns right behind that slot's launch, so that its buffer can be read as the launch left it
 * (airfe_debug_trace_buffer: the first `bytes` bytes of the slot's buffer to the host); -1: run to the end */
int airfe_debug_trace_stop(airfe_ctx* ctx, int slot);
int airfe_debug_trace_buffer(airfe_ctx* ctx, int slot, void* host, size_t bytes);
int airfe_debug_trace_slots(airfe_ctx* ctx);
int airfe_debug_trace_slot(airfe_ctx* ctx, int i, char* name, int name_cap, unsigned* off, unsigned* units, unsigned* unit_words);
int airfe_debug_trace_read(airfe_ctx* ctx, void* stream, unsigned long long* digests, unsigned long long* table);
/* ---- the kernels' workgroup primitives (csrc/wg_prims.h) alone, in ONE workgroup of `threads` (64, 256 or 1024) threads (tests/test_gpu_wg_prims.py).  The workgroup
 * walks v [n] and keep [n] (0 / 1) in rounds of `threads` with a running base, as the production loops do: scan [n] = the exclusive prefix sum of v, pos [n] = the kept
 * entries before each entry; totals [5] = sum of v by the scan, kept entries, then block_sum / block_max / block_min of v (INT32_MIN / INT32_MAX when n = 0); wave
 * [threads / 64][3] = wave_sum / wave_max / wave_min of the first round's values, 0 past n.  keys [P] (key_bytes 4 or 8, unsigned; P = 0 or a power of two with
 * P * key_bytes <= 32768) come back ascending in sorted [P]. */
typedef struct airfe_debug_wg_prims_args {
  const int32_t* v; const uint8_t* keep; int n, threads;
  const void* keys; int P, key_bytes;
  int32_t *scan, *pos, *totals, *wave;       /* out */
  void* sorted;                              /* out */
} airfe_debug_wg_prims_args;
int airfe_debug_wg_prims(airfe_ctx* ctx, airfe_debug_wg_prims_args* a);

#ifdef __cplusplus
}
#endif
#endif /* AIRFE_DEBUG_H_ */
