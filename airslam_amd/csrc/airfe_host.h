// airfe — host side of libairfe.so, shared by its translation units: the context (persistent device arena, weights, staging blocks, stage timers),
// error / allocation helpers and the internal entry points of the pipelines.
//   airfe_load.hip    weight-pack loading and slab packing (≙ TensorRT engine build, src/plnet.cpp:24-196), the matcher arena
//   airfe_detect.hip  the detector pipeline (encoder, heads, NMS, top-K, descriptors)
//   airfe_lines.hip   the PLNet line path: its steps, and line_branch_dev / line_tail_dev / line_post_dev composed of them
//   airfe_match.hip   LightGlue / SuperGlue forwards, the fault-hunting trace and the matchers' host / batch entries (with the two *_scores hooks that are those entries)
//   airfe.hip         context life cycle, scratch blocks, host staging, profiling / trace entries, sync and status, the BoW vocabulary and rectification entries
//   airfe_frame.hip   the frame entries (include/airfe.h): detection, PLNet and stereo over host and device images, the stereo keyframe and track / promote /
//                     adopt, with the pieces their queues and read-backs share
//   airfe_assoc.hip   the point / line association entries: AssignPointsToLines, MatchLines
//   airfe_geom.hip    F-RANSAC, PnP, stereo points, track pose, frame optimisation, stereo lines
//   airfe_bowdb.hip   the BoW vector, the keyframe database and its map tables, the relocalisation and loop detection composites (airfe_bowdb.h: the database
//                     struct and the *_queue functions the next two files share with it)
//   airfe_bowmap.hip  the database's map-point id table, the covisibility build, the map-point triangulation and the map-point merge
//   airfe_junction.hip  the junction connections, the database's junction tables, relocalisation's junction term and its composites
//   airfe_debug.hip   the kernel-level test hooks (include/airfe_debug.h): HookStage, the one stream-ordered holder they stage, wait and read back through
#pragma once
#include "../../include/airfe.h"
#include "../../include/airfe_debug.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#include "common.h"

using namespace airfe;


namespace airfe_host {

extern thread_local std::string g_err;

struct Tensor {
  std::vector<int> dims;
  std::vector<float> data;
};
typedef std::map<std::string, Tensor> Pack;

// sqrt(scale * log2 e), scale = 1/sqrt(d_head) = 0.125: folded into BOTH the q and the k projection (weights and biases; rotary is
// linear, so it commutes), so that q.k comes out of the attention MFMA as log2(e) * (q.k) / 8, ready for v_exp_f32 — the product of two
// packed operands, each rounded once, exactly like the unscaled q and k were
constexpr float ATT_QK_FOLD = 0.42466090014400953f;

struct ConvW { uint16_t* w = nullptr; float* b = nullptr; int cin = 0, cout = 0; };
struct LinW { uint16_t* w = nullptr; float* b = nullptr; int K = 0, N = 0, cbt = 0; uint16_t* wf = nullptr; /* the same weights in MFMA fragment order (make_linear) */ };
// One residual block of either matcher: q | k and v projections, attention, out-projection, 512-wide MLP, residual.  LightGlue's cross half has ONE 256-row projection
// for q and k (qk.N = 256: the two sides swap roles); ln_g = nullptr is the ReLU form (SuperGlue: merge, mlp.0 + ReLU, mlp.3), else LayerNorm + GELU.
struct AttnBlock { LinW qk, v, out, ffn0, ffn3; float *ln_g = nullptr, *ln_b = nullptr; };
struct LgLayer { AttnBlock self, cross; };
constexpr int LINE_CAP = 45056;     // unique candidate lines per image: 300 junctions give at most 300 * 299 / 2 = 44850 (min, max) pairs
constexpr int KEEP_CAP = 3 * 128 * 128;
constexpr int JUNC_CAP = 2048;
// One image's stage-0 line tensors (SURVEY.md Appendix A.1 layouts) inside its stage block, in floats; the CHW loi_features of the
// batch-1 / host-supplied path live in their own block (s0_loi): the batched path samples them from the head GEMM's rows instead.
constexpr size_t SG_JUNCS = 0, SG_LP = 600, SG_KEEP = SG_LP + (size_t)KEEP_CAP * 4, SG_MIN = SG_KEEP + KEEP_CAP, SG_MAX = SG_MIN + KEEP_CAP,
                 SG_THIN = SG_MAX + KEEP_CAP, SG_AUX = SG_THIN + 4 * 128 * 128, SG_STRIDE = (SG_AUX + 4 * 128 * 128 + 63) / 64 * 64;


}  // namespace airfe_host
using namespace airfe_host;

// One grow-on-demand device block.  Ownership, one rule: the memory is registered in its context's `allocs` by the reserve() that made it and freed with
// everything else there by airfe_destroy; an owner that dies before its context (airfe_bowdb: its scratch and its persistent tables alike, airfe_bowdb.h)
// hands its blocks back with release().
struct DevBlock {
  uint8_t* p = nullptr; size_t bytes = 0;
  hipStream_t last = nullptr;    // the stream the block was last handed out for (reserve): synchronised before the block is replaced
  template <class T> T* at(size_t o) const { return reinterpret_cast<T*>(p + o); }
};
struct airfe_ctx;
// st = the stream the caller is about to use the block on (one stream at a time per entry and context: the contract of every *_dev entry).  Grows by
// replacement, only when bytes > b.bytes and only behind a synchronisation of the context's stream and of b.last; no synchronisation otherwise.
int reserve(airfe_ctx* c, DevBlock& b, size_t bytes, hipStream_t st);      // airfe.hip
void release(airfe_ctx* c, DevBlock& b);                                    // airfe.hip
// A block's arrays in two phases: take() while sizing (every part starts on a 256-byte boundary, sizes in size_t), into() reserves the block, then at<T>() / i() /
// d() address the parts.  over() is into() for memory of size() bytes that is no DevBlock (the sequence driver's pinned staging).
struct Carve {
  size_t off = 0; uint8_t* base = nullptr;
  size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; }
  size_t size() const { return off; }
  int into(airfe_ctx* c, DevBlock& b, hipStream_t st) { if (reserve(c, b, off, st)) return 1; base = b.p; return 0; }
  void over(uint8_t* p) { base = p; }
  template <class T> T* at(size_t o) const { return reinterpret_cast<T*>(base + o); }
  int* i(size_t o) const { return at<int>(o); }
  double* d(size_t o) const { return at<double>(o); }
};

// airfe_stereo_keyframe's captured queue (one configuration at a time) and the host-side flags that describe what the queue leaves on the device
struct KfState {
  bool nms_map_valid, desc_normalised, desc_dense_valid, line_sparse; int last_B;
  void save(const airfe_ctx* c);
  void restore(airfe_ctx* c) const;
};
struct KfGraph {
  struct Key {
    int h, w, stride, capL, capJ; bool want_j, match; const void *pin, *blk, *img;
    bool operator==(const Key& o) const {
      return h == o.h && w == o.w && stride == o.stride && capL == o.capL && capJ == o.capJ && want_j == o.want_j && match == o.match && pin == o.pin &&
             blk == o.blk && img == o.img;
    }
  } key{};
  hipGraphExec_t exec = nullptr;
  int seen = 0;
  KfState state{};
  void reset() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; seen = 0; }
};
// What dalloc / dupload / make_linear read of a context: its allocation list and the storage type make_linear packs for (set by each load_* before it packs).  A context
// is one; a test hook's HookStage (airfe_debug.hip) owns a small one of its own, so that no hook needs a whole context to hold its allocations.
struct DevAllocs {
  std::vector<void*> allocs;
  int pack_prec = 0;
};
struct airfe_ctx : DevAllocs {
  airfe_cfg cfg;
  std::string err;
  std::string launch_err;        // cfg.check_launches: the first failed launch since the last report, with its stage's name (launch_status())
  int fail_stage = -1;           // airfe_debug_fail_next_launch: the next ProfScope of this stage makes a deliberately invalid launch first (tests)
  void* copy_ring = nullptr;     // airfe_copy_rows_dev: host-mapped ring of job lists (csrc/airfe_seq.hip)
  int copy_ring_cap = 0, copy_ring_slot = 0, copy_wgs = 64;   // airfe_tuning::copy_wgs
  int *sat_host = nullptr, *sat_flag = nullptr;   // two words of host-mapped, coherent memory (and their device address): [0] = non-finite detector logits, [1] = non-finite
                                 // sampled descriptor — written by the head / sampling kernels only when the 2-byte activations overflowed, read by the host after its synchronisation: no copy
  bool fuse_dec = true;          // airfe_tuning::fuse_dec
  int assign_fused = 0;          // airfe_tuning::assign_fused (1: partials in the similarity tiles; measured -0.010 ms per 64-pair step, +0.012 ms per batch-1 keyframe: not the default, profiles/r05_assign_ab.txt)
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;         // airfe_stereo_plnet_batch_dev: the line branch runs here while the matcher runs on the caller's stream
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_feat = nullptr;
  bool overlap_lines = true;             // line path on stream2 beside the matcher (airfe_stereo_plnet_batch_dev); airfe_tuning::overlap_lines = 0: one stream
  int prec = 0;                  // detector storage type
  int mprec = 1;                 // matcher storage type (cfg.matcher_precision)
  int Bmax = 1, chunk = 1, Np = 64, Pmax = 1;
  int lgb_tokens = 0;            // airfe_tuning::lgb_tokens: forces the fused block's tokens per workgroup (32 / 64 / 112 / 128)
  // batch-1 host entries: ONE pinned host block and contiguous device blocks, so that a call is one H2D and one D2H (the reference's
  // BufferManager does a cudaMalloc + one synchronous memcpy per binding and call: 3rdparty/tensorrtbuffer/include/buffers.h:237-417)
  uint8_t* pin = nullptr;        // hipHostMalloc'ed
  size_t pin_bytes = 0;
  uint8_t *io_in = nullptr, *io_out = nullptr;   // device: [n0 n1 .. | feat0 | feat1] and [nmatch .. | idx | score]
  bool trace_overflow = false;   // a trace slot was dropped (table full): trace_finish fails instead of mis-numbering launches
  size_t arena_rows = 0;         // token rows of the matcher arena, slack included (alloc_matcher_arena)
  int Dmax = 1;                  // images the detector arena holds: 2 x Bmax when a stereo step detects left and right as one batch
  bool has_sp = false, has_lg = false;
  DevBlock pl_stage;             // staging of airfe_assign_points_to_lines / airfe_match_lines
  DevBlock pl_scratch, ml_scratch;   // scratch of airfe_assign_points_to_lines_batch_dev (counts) / airfe_match_lines_batch_dev (bit rows, row maxima): one each
  DevBlock fr_scratch;           // airfe_fundamental_ransac_batch_dev: per-model scores [B][1000][3] + state [B][4]
  DevBlock fr_stage;             // airfe_fundamental_ransac: the one pair's rows and list on the device
  DevBlock pn_scratch;           // airfe_pnp_ransac_batch_dev: per-sample scores [B][100] + models [B][100][12]
  DevBlock pn_gather;            // airfe_track_pose_batch_dev: the gathered correspondences (pnp_gather_queue)
  DevBlock pn_stage;             // airfe_pnp_ransac: the one problem on the device
  DevBlock po_stage;             // airfe_frame_optimize: the one problem on the device
  DevBlock po_gather;            // airfe_track_pose_opt_batch_dev: PnP results, seeds and gathered constraints
  bool outlier_rejection = false;                                       // airfe_set_outlier_rejection: F-RANSAC behind the temporal match of track_frame / stereo_keyframe_tracked
  bool nms_map_valid = true;     // heat_nms holds the last batch's NMS'd maps (large batches skip writing them)
  int Lmax = 1;                  // images the line-path arena holds (= Dmax)
  bool desc_normalised = false;  // dense descriptor map currently holds F.normalize'd rows (only after the inspection hook)
  int gemm_small_max = 4096, gemm8_min = 16000, gemmr_min = 8192, gemmr_wgs = 256;   // GemmArgs::small_max / g8_min / gr_min / gr_wgs (airfe_tuning::gemm_small_max_m, gemm8_min_m, gemmr_min_m, gemmr_wgs)
  int block_min = 0;             // tokens from which the fused LightGlue block is used (airfe_tuning::block_min_m).  Round 4: with 32- / 64-token passes for small
                                 // token counts the fused kernel wins at EVERY size (profiles/r04_lg_small_batch_sweep.txt: 1 pair 0.70 vs 0.78 ms, 4 pairs 0.75 vs 1.20);
                                 // with 112- / 128-token passes only (rounds 1-3) the four separate launches were quicker below 3200 tokens
  bool qkv_pair = true;          // q|k and v of a layer in one streaming launch (airfe_tuning::qkv_pair = 0: two launches)
  int fuse_lg_block = -1;        // LightGlue out-proj + FFN + residual as one kernel: -1 by token count, airfe_tuning::fuse_lg_block = 0 / 1 forces
  int sg_kenc_gemm = -1;         // airfe_tuning::sg_kenc_gemm = 0 / 1: SuperGlue keypoint encoder's large layers as scalar loops / GEMMs (default: by token count)
  bool desc_dense_valid = true;  // c->desc holds the dense map of the last batch (else: the gather GEMM's rows)
  int last_B = 0;
  int* desc_idx = nullptr;       // row list of the descriptor head's gather GEMM
  int n_cu = 0;                  // compute units of cfg.device (hipDeviceAttributeMultiprocessorCount): the fused block's two-round split
  bool fold_qkv = true;          // airfe_tuning::fold_qkv = 0: q | k | v projections as launches of their own (A/B runs)
  bool desc_gather_stream = true;   // airfe_tuning::desc_gather_stream = 0: the descriptor head over sampled cells in the tiled kernel (gemm8) at every size (A/B, bit-identity test)
  bool fold_out = true;          // airfe_tuning::fold_out_proj: out_proj / to_out / merge multiplied into the message half of ffn.0 / mlp.0 at pack time (2-byte matcher only);
                                 // the packed ffn.0 / mlp.0 of the context then expect cat(x, attention output), and no entry runs the out-projection

  // detector weights
  float *c1a_w = nullptr, *c1a_b = nullptr;
  ConvW c1b, c2a, c2b, c3a, c3b, c4a, c4b, cPa, cDa;
  LinW cPb, cDb;
  // detector arena
  float* img32 = nullptr;
  uint16_t *a1b = nullptr, *a2a = nullptr, *a2b = nullptr, *a3a = nullptr, *a3b = nullptr, *a4a = nullptr,
           *a4b = nullptr, *aPa = nullptr, *aDa = nullptr;
  float *logits = nullptr, *heat = nullptr, *heat_nms = nullptr, *nms_tmp = nullptr, *desc = nullptr;
  unsigned char* nms_mask = nullptr;   // max_mask + supp_mask planes of the per-pool NMS launches
  int *xtab = nullptr, *ytab = nullptr;
  float* lut = nullptr;
  unsigned long long* cand = nullptr;   // [Bmax][512*512] detect_point candidate keys
  int* cand_cnt = nullptr;
  int tab_w = -1, tab_h = -1;
  // BoW vocabulary tree
  float *bow_desc = nullptr, *bow_weight = nullptr, *bow_outw = nullptr;
  std::vector<double> bow_weight_h;   // the vocabulary's WordValue weights as the reference holds them (double): the host entry returns these
  int* bow_outn = nullptr;            // leaf node per feature of the last host call
  int *bow_first = nullptr, *bow_nch = nullptr, *bow_word = nullptr;
  unsigned* bow_out = nullptr;
  int bow_nodes = 0;
  double* bow_weight_d = nullptr;     // the same weights on the device: the BoW vector's sums are double (airfe_bow_vector_batch_dev)
  int bow_nwords = 0;                 // 1 + the largest word id
  DevBlock bv_scratch;                // airfe_bow_vector_batch_dev: word / weight / node per feature
  DevBlock bv_stage;                  // airfe_bow_vector: the host entry's device block
  // rectification maps of Camera (camera.cc:60-75), one pair per side, and the rectified-image staging
  float* rmap[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  int rmap_h[2] = {0, 0}, rmap_w[2] = {0, 0};
  DevBlock st_rect;
  // host-API staging
  DevBlock st_img;
  DevBlock kf_blk;                                  // airfe_stereo_keyframe's device block (grows on demand)
  DevBlock tk_blk, ref_blk;                         // airfe_track_frame: outputs; the last keyframe's features
  int ref_n = -1;
  int tk_n = -1;                                    // keypoints of the last airfe_track_frame's frame (its rows are still in tk_blk); -1: none
  DevBlock pr_blk;                                  // airfe_promote_frame: [counts | right rows | idx | score]
  int kf_spec_lines = 1024, kf_spec_juncs = 512;   // line / junction rows airfe_stereo_keyframe copies back before it knows the counts (airfe_tuning::kf_spec_rows)
  bool kf_graph_on = false;                         // airfe_tuning::kf_graph
  KfGraph kf_graph;
  float *st_feat0 = nullptr, *st_feat1 = nullptr, *st_score = nullptr;
  int *st_n0 = nullptr, *st_n1 = nullptr, *st_nm = nullptr;
  int32_t* st_idx = nullptr;
  float* st_scores_full = nullptr;

  // LightGlue
  std::vector<LgLayer> lg;
  LinW lg_final;
  float *lg_wr = nullptr, *lg_mw = nullptr;
  float lg_mb = 0.f;
  float *x32 = nullptr, *rot_cos = nullptr, *rot_sin = nullptr, *zbuf = nullptr, *simbuf = nullptr, *rowlse = nullptr,
        *collse = nullptr, *rowval = nullptr;
  uint16_t *xb = nullptr, *qb = nullptr, *kb = nullptr, *vtb = nullptr, *ob = nullptr, *msg = nullptr, *hb = nullptr,
           *mdb = nullptr;
  int *lens = nullptr, *rowarg = nullptr, *colarg = nullptr;
  float *lg_part = nullptr, *lg_argpart = nullptr;   // [Pmax][2][tiles][Np] float2 each: launch_lg_assign_fused
  bool has_arena = false;

  // SuperGlue
  bool has_sg = false;
  std::vector<AttnBlock> sg;
  LinW sg_final;
  float sg_alpha = 1.f;
  const float* sg_kenc[10] = {nullptr};
  LinW sg_k3, sg_k4;             // keypoint-encoder layers 3 (128 -> 256) and 4 (256 -> 256) for the GEMM path
  int Lz = 0;
  float *sg_u = nullptr, *sg_v = nullptr, *sg_Z = nullptr, *sg_max0 = nullptr, *sg_ms0 = nullptr, *sg_ms1 = nullptr;
  int *sg_idx0 = nullptr, *sg_idx1 = nullptr;
  float* sg_xch = nullptr;       // [P][2][16][Lz] (max, sum) column partials of the register-resident Sinkhorn kernel
  unsigned* sg_cnt = nullptr;    // per-pair rendezvous counters of the fused Sinkhorn kernel
  int32_t *sg_out0 = nullptr, *sg_out1 = nullptr;

  // fp32 correctness path (cfg.precision = 2 / matcher_precision = 2): fp32 weights and activations, kernels_f32.hip
  struct F32Conv { float* w = nullptr; float* b = nullptr; int cin = 0, cout = 0; };
  struct F32Lin { float* w = nullptr; float* b = nullptr; int K = 0, N = 0; };
  // AttnBlock in fp32.  An absent v (v.w = nullptr) means v's rows are in qk: ONE 768-row q | k | v matrix, rows head-major (LightGlue's self half, SuperGlue, whose
  // out-projection also has its input columns head-major); LightGlue's cross half has its 256-row q = k matrix and v.
  struct F32Block { F32Lin qk, v, out, ffn0, ffn3; float *ln_g = nullptr, *ln_b = nullptr; };
  struct F32LgLayer { F32Block self, cross; };
  F32Conv f_c1b, f_c2a, f_c2b, f_c3a, f_c3b, f_c4a, f_c4b, f_cPa, f_cDa, f_cL1;
  F32Lin f_cPb, f_cDb, f_cLh, f_lgfinal, f_sgfinal;
  std::vector<F32LgLayer> f_lg;
  std::vector<F32Block> f_sg;
  int f_B = 0;                   // images per pass of the fp32 encoder (its activations are 4 bytes: 2 images at a time)
  float *f1a = nullptr, *f1b = nullptr, *fp1 = nullptr, *f2a = nullptr, *f2b = nullptr, *fp2 = nullptr, *f3a = nullptr, *f3b = nullptr,
        *fp3 = nullptr, *f4a = nullptr, *f4b = nullptr, *fPa = nullptr, *fDa = nullptr, *fL1 = nullptr;
  float *m_qkv = nullptr, *m_ctx = nullptr, *m_msg = nullptr, *m_h = nullptr, *m_md = nullptr;
  // PLNet stage-0 line branch (HAWP-style head on the shared trunk; weights ride in the detector pack as line.*)
  bool has_s0 = false;
  ConvW cL1;                     // line.conv1: 3x3 128 -> 128 on the conv3a features
  LinW cLh;                      // line.head : 1x1 128 -> 145 = loi (128) | md0-2 dis res | jloc0-1 | joffx joffy | thin0-3 | aux0-3
  LinW cLh_loi, cLh_dec;         // the same rows as two heads: the 128 LOI channels (run on the junctions' tap rows only) and the 17 decoded ones
  bool line_sparse = false;      // the last line_branch_dev ran the split heads (else: the fused head over one image, l_head)
  float* l_dec = nullptr;        // [Lmax][128*128][32]: the 17-channel head
  int* l_ridx = nullptr;         // [Lmax * 1200 (+ pad)]: tap rows of the junctions
  float* l_lrows = nullptr;      // [Lmax * 1200 (+ pad)][128]: LOI features of those rows
  uint16_t* l_feat = nullptr;    // [Lmax][128*128][128] 2-byte
  float *l_ta8 = nullptr /*[Lmax][128*128][8] thin | aux pixel-major*/, *l_head = nullptr, *l_jloc = nullptr, *l_joff = nullptr, *l_sel = nullptr;
  int* l_nsel = nullptr;
  unsigned long long* l_cand = nullptr;   // [Lmax][128*128] junction candidates (its own list: the line branch may run beside the point branch's tail)
  int* l_cand_cnt = nullptr;
  // PLNet stage 1 + line path
  bool has_s1 = false;
  const float* s1_w[11] = {nullptr};
  const uint16_t* s1_wsplit[6] = {nullptr};   // fc2.0 (thin / aux columns), fc2_res.0, fc2.2, fc2.4, fc2.0's LOI columns of end point 1 / 2 as fp16 (hi, lo) planes
  int *wf_table = nullptr, *wf_keep = nullptr, *wf_pairs = nullptr, *wf_rep = nullptr, *wf_counts = nullptr;
  bool wf_counted = false;                     // the stage block's per-workgroup keep counts are in wf_counts (launch_s0_j2l wrote them): launch_wireframe skips its count pass
  float* wf_prop = nullptr;                    // [L][LINE_CAP][4]: lines_pred of every unique line's first proposal (wireframe_kernel -> plnet_s1h_kernel)
  float *s1_la = nullptr, *s1_sc = nullptr, *s1_jfeat = nullptr /*[Lmax][300][256]*/, *s0_stage = nullptr /*[Lmax][SG_STRIDE]*/, *s0_loi = nullptr /*CHW [128][128][128], one image*/,
        *junc_feat = nullptr;
  unsigned char* jmap = nullptr;
  double* d_lines = nullptr;
  int *d_nlines = nullptr /*[Lmax] kept | [Lmax] found*/, *d_njunc = nullptr /*[Lmax] kept | [Lmax] found | [Lmax][64] scan scratch*/;

  // fault hunting (airfe_debug_trace*): checksums of the matcher's state behind every launch of lightglue_dev
  struct TraceSlot { std::string name; unsigned off, units, unit_words; const void* p; size_t words; };
  bool trace_on = false, trace_halt = false;
  int trace_stop = -1;           // >= 0: the forward pass returns right behind this slot (its buffer stays as that launch left it)
  unsigned long long *trace_tab = nullptr, *trace_dig = nullptr;
  unsigned* trace_off = nullptr;
  size_t trace_cap = 0;
  std::vector<TraceSlot> trace_slots;
  std::vector<unsigned> trace_off_h;

  // per-stage hipEvent timers (airfe_profile_*): events are recorded on the launch stream only
  struct Mark { int stage; hipEvent_t a, b; double flops, bytes; };
  uint32_t prof_mask = 0;        // bit i = stage i is bracketed by events
  std::vector<Mark> marks;
  std::vector<hipEvent_t> ev_pool;
};

// the stream a *_dev entry queues on: the caller's, or the context's when the caller passes none
inline hipStream_t stream_of(const airfe_ctx* c, void* stream) { return stream ? static_cast<hipStream_t>(stream) : c->stream; }

enum Stage {
  ST_PREPROCESS = 0, ST_CONV1_FUSED /* conv1a + conv1b + pool: the dominant kernel, its own stage */, ST_CONV3X3_C64, ST_CONV3X3_C128, ST_HEAD_GEMM, ST_HEAD_ELTWISE, ST_NMS, ST_SELECT,
  ST_SAMPLE, ST_LG_PREPARE, ST_LG_GEMM, ST_LG_ATTENTION, ST_LG_LNGELU, ST_LG_ASSIGN, ST_PL_DECODE, ST_PL_STAGE1, ST_PL_FILTER, ST_LINE_ASSOC, ST_RECTIFY, ST_BOW, ST_COUNT
};
static const char* kStageNames[ST_COUNT] = {
  "preprocess", "conv1_fused", "conv3x3_cin64", "conv3x3_cin128", "head_gemm", "head_eltwise", "simple_nms", "select_topk",
  "sample_desc", "lg_prepare", "lg_gemm", "lg_attention", "lg_ln_gelu", "lg_assign", "plnet_s0_decode", "plnet_stage1", "plnet_filter", "line_assoc", "rectify", "bow"};

void note_launch(airfe_ctx* c, int stage);      // airfe.hip
void fail_launch_now(hipStream_t st);            // airfe.hip: a deliberately invalid launch (airfe_debug_fail_next_launch)
struct ProfScope {
  airfe_ctx* c; hipStream_t st; bool on; int stage; airfe_ctx::Mark m;
  ProfScope(airfe_ctx* c_, int stage_, hipStream_t st_, double flops, double bytes) : c(c_), st(st_), on((c_->prof_mask >> stage_) & 1u), stage(stage_) {
    if (c->fail_stage == stage) { c->fail_stage = -1; fail_launch_now(st); if (c->cfg.check_launches) note_launch(c, stage); }
    if (!on) return;
    auto get = [&]() {
      hipEvent_t e;
      if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); }
      else (void)hipEventCreate(&e);
      return e;
    };
    m.stage = stage; m.flops = flops; m.bytes = bytes; m.a = get(); m.b = get();
    (void)hipEventRecord(m.a, st);
  }
  ~ProfScope() {
    if (c->cfg.check_launches) note_launch(c, stage);      // the launches of this stage: reported by launch_status() with the stage's name
    if (!on) return;
    (void)hipEventRecord(m.b, st);
    try { c->marks.push_back(m); } catch (...) { c->ev_pool.clear(); }      // (a destructor must not throw; the events leak rather than the process die)
  }
};

namespace airfe_host {

#define HIPCHK(ctx, expr)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                             \
      g_err = (ctx)->err;                                                                         \
      return 1;                                                                                   \
    }                                                                                             \
  } while (0)

int fail(airfe_ctx* c, const std::string& m);
int fail_noexcept(airfe_ctx* c, const char* what, const char* detail) noexcept;   // for the catch blocks at the C boundary
// 0 when no launch failed since the last report; else the context's error = "<stage>: kernel launch failed: <hip error>" and 1.  With
// cfg.check_launches every stage's launches are looked at as the stage ends (ProfScope); without it this is one hipGetLastError().
int launch_status(airfe_ctx* c);
// Reads and clears the detector's saturation words (after the caller's synchronisation): non-zero -> the context's error says that the 2-byte activations left the
// fp16 / bf16 range and 1 is returned — never keypoints of a poisoned score map.
int saturation_status(airfe_ctx* c);

template <class T>
T* dalloc(DevAllocs* c, size_t n, bool zero = true) {
  void* p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
  if (zero) (void)hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T));
  c->allocs.push_back(p);
  return reinterpret_cast<T*>(p);
}
template <class T>
T* dupload(DevAllocs* c, const std::vector<T>& v) {
  T* p = dalloc<T>(c, v.size(), false);
  if (p && !v.empty()) (void)hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return p;
}

// ---- airfe_load.hip
int load_superpoint(airfe_ctx* c, const char* path);
int load_lightglue(airfe_ctx* c, const char* path);
int load_superglue(airfe_ctx* c, const char* path);
int load_plnet_s1(airfe_ctx* c, const char* path);
std::vector<int> resize_table(int dsize, int ssize);
std::vector<uint16_t> pack_slabs(int cbt, int nslab, int prec, const std::function<float(int, int, int)>& get);
uint16_t f2bf(float f);
uint16_t f2h(float f);
float h2f(uint16_t h);
inline uint16_t cvt2(float f, int prec) { return prec == 1 ? f2h(f) : f2bf(f); }
inline float back2(uint16_t v, int prec) {
  if (prec == 1) return h2f(v);
  uint32_t u = (uint32_t)v << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
bool make_linear(DevAllocs* c, const float* W, const float* bias, int K, int N, LinW& out, float scale = 1.f,
                 const std::function<int(int)>* src_row = nullptr, const std::function<int(int)>* src_col = nullptr);
// ---- airfe_detect.hip
int ensure_tables(airfe_ctx* c, int h, int w);
int run_conv(airfe_ctx* c, const ConvW& w, const uint16_t* x, uint16_t* y, int B, int H, int W, int pool, int out_pad, hipStream_t st);
int dense_desc_head(airfe_ctx* c, int B, hipStream_t st);
int detect_tail_dev(airfe_ctx* c, int B, int Bs, bool two, bool sparse_desc, int h, int w, float* d_feat, float* d_feat1, int cap, int* d_n, int* d_n1,
                    hipStream_t st);
int detect_dev2(airfe_ctx* c, const uint8_t* d_gray, const uint8_t* d_gray1, int Bs, int h, int w, int stride, size_t img_stride,
                float* d_feat, float* d_feat1, int cap, int* d_n, int* d_n1, hipStream_t st);
int detect_dev(airfe_ctx* c, const uint8_t* d_gray, int B, int h, int w, int stride, size_t img_stride, float* d_feat, int cap, int* d_n, hipStream_t st);
int point_desc_head(airfe_ctx* c, int B, int cap, hipStream_t st, bool& sparse);      // the sparse / dense descriptor-head decision, the dense head, desc_dense_valid and last_B
// ---- airfe_lines.hip: the line path's steps (production's compositions below and the test hooks call the same ones)
void junctions_topk_dev(airfe_ctx* c, int nb, hipStream_t st);
void line_head_gemm(airfe_ctx* c, int nb, bool fused, int prec, const LinW& hw, hipStream_t st);
void line_head_decode(airfe_ctx* c, int nb, int prec, const LinW& hw, float* jnms, int wgs, hipStream_t st);
void line_decode_rows(airfe_ctx* c, int nb, const float* head, int ld, int off, float* jnms, bool ta8, bool loi_chw, hipStream_t st);
void line_match(airfe_ctx* c, int nb, bool exact_all, hipStream_t st);
void line_dedup(airfe_ctx* c, int nb, hipStream_t st);
int line_tap_rows(airfe_ctx* c, int nb, hipStream_t st);
void line_loi_rows(airfe_ctx* c, int nb, hipStream_t st);
// stage 1's LOI source and operand form.  0 .. 3 are airfe_debug_line_mid's s1_form (include/airfe_debug.h); S1_HEAD_H is fp32 mode with cfg.line_precision = 3.
enum S1Form { S1_CHW = 0, S1_HEAD = 1, S1_ROWS = 2, S1_ROWS_H = 3, S1_HEAD_H = 4 };      // CHW tensors | head rows | gathered rows, fp32 | gathered rows, fp16 pairs | head rows, fp16 pairs
void line_stage1(airfe_ctx* c, int nb, int form, int wgs, hipStream_t st);
void junction_maps_clear(airfe_ctx* c, int nj, hipStream_t st);
void line_filter_maps(airfe_ctx* c, int nb, int nj, int h, int w, double* d_lines, int capL, int* d_nlines, int* d_lfound, hipStream_t st);
int junction_scan_maps(airfe_ctx* c, int i0, int nj, float* d_junc, int capJ, int* d_njunc, int* d_jfound, hipStream_t st);
int junction_desc_sample(airfe_ctx* c, int i0, int nj, int h, int w, float* d_junc, int capJ, const int* d_njunc, hipStream_t st);
int junction_dense_maps(airfe_ctx* c, int nj, int capJ, int phase, hipStream_t st, bool& partial);
int line_branch_dev(airfe_ctx* c, hipStream_t st, int i0, int nb, bool chw);
int line_tail_dev(airfe_ctx* c, int i0, int nb, bool host_s0, int h, int w, double* d_lines, int capL, int* d_nlines, int* d_lfound,
                  float* d_junc, int capJ, int* d_njunc, int* d_jfound, int nj, hipStream_t st, int phase = 3);
bool junction_tail_fused(airfe_ctx* c, int nj, int capJ);      // the junction list inside the line filter + the descriptors from the sampling gather GEMM (no dense maps)
int line_post_dev(airfe_ctx* c, int i0, int nb, int h, int w, double* d_lines, int capL, int* d_nlines, int* d_lfound, float* d_junc, int capJ, int* d_njunc,
                  int* d_jfound, int nj, hipStream_t st, int phase, bool fused);
// ---- airfe_match.hip
void trace(airfe_ctx* c, hipStream_t st, const char* what, size_t li, const char* blk, const void* p, size_t words, unsigned unit_words);
int trace_finish(airfe_ctx* c, hipStream_t st);
int run_linear(airfe_ctx* c, const LinW& w, const uint16_t* x1, int ld1, int K1, const uint16_t* x2, int ld2, int M, int epi, int act, void* out,
                int ldo, hipStream_t st, bool trans = false, void* out2 = nullptr, float* x32 = nullptr, const float* rc = nullptr, const float* rs = nullptr);
int sg_front_dev(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int normalize, bool split, hipStream_t st);
struct LgSecondPair { const float *f0, *f1; const int *n0, *n1; };      // a second pair for a B = 1 call (same ld / kp_off / normalize): outputs of pair 1 follow pair 0's
int lightglue_dev(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int ld, int kp_off, int normalize,
                  int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, float* scores_out, hipStream_t st, const LgSecondPair* x2 = nullptr);
int superglue_dev(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int normalize, hipStream_t st);
int sinkhorn_failed(airfe_ctx* c);      // a Sinkhorn rendezvous of an earlier SuperGlue call timed out (read after a synchronisation, cleared once reported)

}  // namespace airfe_host

// ---- every file with C entries
// Every extern "C" entry is a function-try-block ending in AIRFE_CATCH: std::bad_alloc from a std::vector / std::string of the host-side
// bookkeeping (or anything else thrown below) becomes a non-zero return + airfe_last_error(), never an exception crossing the C ABI.
#define AIRFE_CATCH(c)                                                                                                   \
  catch (const std::exception& e_) { return airfe_host::fail_noexcept((c), __func__, e_.what()); }                       \
  catch (...) { return airfe_host::fail_noexcept((c), __func__, nullptr); }
// Every entry that takes a context makes the context's device current first: a process may hold contexts on several devices (cfg.device)
// and the calling thread's current device is whatever the application left it at.
inline int enter_device(airfe_ctx* c) {
  int d = -1;
  if (hipGetDevice(&d) == hipSuccess && d == c->cfg.device) return 0;
  if (hipSetDevice(c->cfg.device) != hipSuccess) return fail(c, "hipSetDevice(cfg.device) failed");
  return 0;
}
#define AIRFE_ENTER(c) do { if (!(c)) return 1; if (enter_device(c)) return 1; } while (0)
// ---- airfe.hip
int ensure_pin(airfe_ctx* c, size_t bytes);
int upload_image(airfe_ctx* c, const uint8_t* gray, int h, int w, int stride);
// A host entry that returns with an error AFTER it queued work must not leave that work in flight: the next call memcpy's into the pinned block a
// pending D2H may still write, and reference rows that were only partly uploaded must not be matched against.  Armed once queueing starts,
// disarmed on success.
// A host entry reports the overflow of ITS OWN call: a saturation word an earlier asynchronous *_batch_dev call left behind (whose caller never asked: airfe_sync /
// airfe_superglue_status) must not fail a later healthy call with a stale "left the fp16 range" (ADVICE r05).  Cleared where a host entry starts queueing.
inline void clear_saturation(airfe_ctx* c) {
  if (c->sat_host) c->sat_host[0] = c->sat_host[1] = 0;
}
struct DrainOnError {
  airfe_ctx* c; bool armed = false, ref_uploaded = false;
  explicit DrainOnError(airfe_ctx* c_, bool armed_ = false) : c(c_), armed(armed_) { clear_saturation(c_); }
  ~DrainOnError() {
    if (!armed) return;
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->stream2);
    if (ref_uploaded) c->ref_n = -1;
  }
};
// ---- the pinned block's read-backs, after the wait that brought them home (airfe_frame.hip, airfe_match.hip)
// [counts | rows of image 0 | rows of image 1 ..] at the start of the pinned block, max_keypoints rows per image: image img's rows -> feat; returns how many
inline int rows_out(const airfe_ctx* c, int img, float* feat) {
  const int Np = c->cfg.max_keypoints, n = std::min(reinterpret_cast<const int*>(c->pin)[img], Np);
  if (n > 0) memcpy(feat, c->pin + 64 + (size_t)img * Np * AIRFE_FEAT_DIM * 4, (size_t)n * AIRFE_FEAT_DIM * 4);
  return n;
}
// [idx | score] at c->pin + off -> nm matches of the pair whose list starts at row `first`; stride = the bytes of the idx part (Np * 8 for one pair, Np * 16 for
// the keyframe's two)
inline void matches_out(const airfe_ctx* c, size_t off, size_t stride, int first, int nm, int32_t* idx, float* score) {
  if (nm < 1) return;
  memcpy(idx, c->pin + off + (size_t)first * 8, (size_t)nm * 8);
  memcpy(score, c->pin + off + stride + (size_t)first * 4, (size_t)nm * 4);
}
// ---- airfe_frame.hip: what the batch-1 frame entries' queues share
// [count | n_ref rows] through the pinned block at `off` into ref_blk, queued on st.  The stored count becomes valid with the queued upload; drain takes it back
// if the call fails before the stream is idle.
int upload_reference(airfe_ctx* c, DrainOnError& drain, size_t off, const float* ref_feat, int n_ref, hipStream_t st);
// the first `bytes` of a frame entry's device block ([counts | feature rows]) go home to the start of the pinned block on s2; ev_feat marks their arrival
int rows_home(airfe_ctx* c, const DevBlock& blk, size_t bytes, hipStream_t s2);
// the second (and last) round trip of a PLNet host entry: line / junction rows, whose counts are known only after the first wait, through the pinned block
struct RowsPart { const void* dev; void* host; size_t bytes; };
int rows_second_trip(airfe_ctx* c, std::initializer_list<RowsPart> parts, hipStream_t st);
int upload_stage0(airfe_ctx* c, const airfe_plnet_stage0* s0, hipStream_t st);      // caller-supplied stage-0 tensors -> stage slot 0 + the CHW LOI block
// ---- airfe_geom.hip: the pipelines on a stream, queued by their own entries, by the keyframe / track entries and by the composites of airfe_bowdb.hip
int fransac_queue(airfe_ctx* c, const float* d_f0, const float* d_f1, int B, int cap, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, double* d_F,
                  hipStream_t st);
int pnp_queue(airfe_ctx* c, const float* d_obj, const float* d_img, const int* d_n, int B, int ncap, const double* K, double* d_Twc, double* d_Rt, uint8_t* d_mask,
              int mcap, const int* d_map, int* d_count, hipStream_t st);
int poseopt_queue(airfe_ctx* c, const double* d_X, const double* d_obs, const int* d_n, int B, int ncap, const double* d_Twc0, const double* cam, const double* Tcb,
                  const double* thr, double* d_Twc, double* d_Rt, uint8_t* d_inlier, int mcap, const int* d_map, int* d_num, int lost, int* d_ok, hipStream_t st);
int stereo_lines_queue(airfe_ctx* c, const double* cam, const double* d_left, const int* d_nl, const double* d_right, const int* d_nr, int capL,
                       const int32_t* d_matches, const double* d_Twc, int B, double* d_sel, uint8_t* d_valid, int32_t* d_status, double* d_endpoints,
                       double* d_plucker, int32_t* d_count, hipStream_t st);
