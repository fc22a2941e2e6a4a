// airfe — LightGlue / SuperGlue forwards on device-resident features, the fault-hunting trace and the matchers' host and batch entries (see airfe_host.h)
#include "airfe_host.h"

namespace airfe_host {

// PointMatcher::NormalizeKeypoints (src/point_matcher.cc:39-48): integer width / 2 and height / 2, L_inv = 1.0 / max(w, h) * scale (0.5 for LightGlue, 0.7 for
// SuperGlue: point_matcher.cc:58)
struct KpNorm { float cx, cy, linv; };
static KpNorm kp_norm(const airfe_ctx* c, float scale) {
  return {(float)(c->cfg.image_width / 2), (float)(c->cfg.image_height / 2), (float)(1.0 / std::max(c->cfg.image_width, c->cfg.image_height) * (double)scale)};
}

// launch_lg_prepare's arguments for B pairs into the context's arena; the caller adds the slack rows it wants back at zero (and a second pair)
static LgPrepArgs lg_prep_args(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int ld, int kp_off, int normalize) {
  const KpNorm k = kp_norm(c, 0.5f);
  LgPrepArgs pa;
  pa.f0 = f0; pa.f1 = f1; pa.n0 = n0; pa.n1 = n1; pa.ld = ld; pa.kp_off = kp_off; pa.normalize = normalize;
  pa.cx = k.cx; pa.cy = k.cy; pa.linv = k.linv;
  pa.wr = c->lg_wr; pa.B = B; pa.cap = cap; pa.Np = c->Np;
  pa.x32 = c->x32; pa.xb = c->xb; pa.rot_cos = c->rot_cos; pa.rot_sin = c->rot_sin; pa.lens = c->lens;
  return pa;
}

// SuperGlue's optimal-transport tail on the context's buffers: Sinkhorn in log space over simbuf, then the decode
static void sg_transport_dev(airfe_ctx* c, int B, hipStream_t st) {
  launch_sg_sinkhorn(c->simbuf, c->lens, B, c->Np, c->Lz, c->sg_alpha, c->cfg.sinkhorn_iters, c->sg_u, c->sg_v, c->sg_Z, c->sg_cnt, c->sg_cnt + (size_t)c->Pmax * 16, c->sg_xch, st);
  launch_sg_decode(c->sg_Z, c->lens, B, c->Np, c->Lz, 0.2f, c->sg_idx0, c->sg_max0, c->sg_idx1, c->sg_out0, c->sg_out1, c->sg_ms0, c->sg_ms1, st);
}

// ---- the fp32 forwards (cfg.matcher_precision = 2; same call contracts as lightglue_dev / superglue_dev)
// y [M][w.N] = (cat(x1, x2) W^T + b) * scale over the arena's rows (x1 alone has all of w.K columns; with x2 each has 256), ReLU'd / added to y where asked
static void lin_f32(airfe_ctx* c, int M, hipStream_t st, const airfe_ctx::F32Lin& w, const float* x1, const float* x2, float* y, int ldy, int acc = 0, int relu = 0,
                    float scale = 1.f) {
  GemmF32Args g;
  g.X1 = x1; g.ld1 = g.K1 = x2 ? 256 : w.K; g.X2 = x2; g.ld2 = x2 ? 256 : 0; g.W = w.w; g.bias = w.b; g.Y = y; g.ldy = ldy;
  g.M = M; g.N = w.N; g.K = w.K; g.accumulate = acc; g.relu = relu; g.scale = scale;
  launch_gemm_f32(g, st);
}
// sim[b] = md[2b] . md[2b+1]^T per pair
static void sim_f32(airfe_ctx* c, int B, hipStream_t st) {
  const int Np = c->Np;
  for (int b = 0; b < B; ++b) {
    GemmF32Args g;
    g.X1 = c->m_md + (size_t)(2 * b) * Np * 256; g.ld1 = 256; g.K1 = 256; g.K = 256; g.W = c->m_md + (size_t)(2 * b + 1) * Np * 256;
    g.Y = c->simbuf + (size_t)b * Np * Np; g.ldy = Np; g.M = Np; g.N = Np;
    launch_gemm_f32(g, st);
  }
}
// One residual block: q | k | v from ONE [768][256] projection with head-major rows — or, LightGlue's cross half, q = k from one 256-row projection and v from its own —,
// rotary where asked, exact soft-max attention, out-projection, the MLP on cat(x, message) (LayerNorm + erf GELU, or ReLU: BatchNorm is folded into mlp.0 in the
// pack), added to x
static void attn_block_f32(airfe_ctx* c, const airfe_ctx::F32Block& b, int S, int cross, bool rotary, hipStream_t st) {
  const int Np = c->Np, M = S * Np;
  lin_f32(c, M, st, b.qk, c->x32, nullptr, c->m_qkv, 768);
  if (b.v.w) lin_f32(c, M, st, b.v, c->x32, nullptr, c->m_qkv + 512, 768);
  if (rotary) launch_rotary_f32(c->m_qkv, 768, c->rot_cos, c->rot_sin, M, st);
  launch_attention_f32(c->m_qkv, 768, b.v.w ? c->m_qkv : c->m_qkv + 256, 768, c->m_qkv + 512, 768, c->m_ctx, c->lens, S, 4, Np, cross, 0.125f, st);
  lin_f32(c, M, st, b.out, c->m_ctx, nullptr, c->m_msg, 256);
  lin_f32(c, M, st, b.ffn0, c->x32, c->m_msg, c->m_h, 512, 0, b.ln_g ? 0 : 1);
  if (b.ln_g) launch_ln_gelu_f32(c->m_h, b.ln_g, b.ln_b, M, st);
  lin_f32(c, M, st, b.ffn3, c->m_h, nullptr, c->x32, 256, 1);
}

// LightGlue: self (rotary) and cross half per layer; final_proj with d^-1/4 on both sides (d = 256); the assignment tail is the shared fp32 code
static int lightglue_dev_f32(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int ld, int kp_off, int normalize,
                             int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, float* scores_out, hipStream_t st) {
  const int S = 2 * B, Np = c->Np, M = S * Np;
  LgPrepArgs pa = lg_prep_args(c, f0, n0, f1, n1, B, cap, ld, kp_off, normalize);
  pa.slack_rows = (int)(c->arena_rows - (size_t)M);      // the slack rows go back to zero with the same launch (see reset_slack_rows)
  launch_lg_prepare(1, pa, st);
  for (const auto& l : c->f_lg) {
    attn_block_f32(c, l.self, S, 0, true, st);
    attn_block_f32(c, l.cross, S, 1, false, st);
  }
  lin_f32(c, M, st, c->f_lgfinal, c->x32, nullptr, c->m_md, 256, 0, 0, 0.25f);
  launch_rowdot256(c->x32, c->lg_mw, c->lg_mb, c->zbuf, M, st);
  sim_f32(c, B, st);
  launch_lg_assign(c->simbuf, c->zbuf, c->lens, B, Np, mcap, 0.1f, c->rowlse, c->collse, scores_out, c->rowarg, c->rowval, c->colarg, d_idx,
                   d_score, d_nmatch, st);
  return launch_status(c);
}

// SuperGlue: keypoint encoder as fp32 FMA loops (the prepare kernel's unsplit form), GNN layers self / cross alternating (names = ['self', 'cross'] * 9), final_proj with
// scores / 256^.5 split over both sides; the optimal-transport tail is the shared fp32 code
static int superglue_dev_f32(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int normalize, hipStream_t st) {
  const int S = 2 * B, Np = c->Np, M = S * Np;
  if (sg_front_dev(c, f0, n0, f1, n1, B, cap, normalize, false, st)) return 1;
  int li = 0;
  for (const auto& l : c->f_sg) attn_block_f32(c, l, S, li++ & 1, false, st);
  lin_f32(c, M, st, c->f_sgfinal, c->x32, nullptr, c->m_md, 256, 0, 0, 0.25f);
  sim_f32(c, B, st);
  sg_transport_dev(c, B, st);
  return launch_status(c);
}

// airfe_debug_trace: checksum `words` 32-bit words of p in units of unit_words (slot = one call; no-op unless tracing)
void trace(airfe_ctx* c, hipStream_t st, const char* what, size_t li, const char* blk, const void* p, size_t words, unsigned unit_words) {
  if (!c->trace_on) return;
  const unsigned off = c->trace_slots.empty() ? 0u : c->trace_slots.back().off + c->trace_slots.back().units;
  const unsigned units = (unsigned)(words / unit_words);
  if (units == 0) return;                                          // nothing to hash (and a 0-sized grid is a launch error)
  if (c->trace_slots.size() >= 1024 || (size_t)off + units > c->trace_cap) { c->trace_overflow = true; return; }   // reported by trace_finish
  launch_trace_hash(p, unit_words, units, c->trace_tab + off, st);
  c->trace_slots.push_back({std::string("L") + std::to_string(li) + "." + blk + "." + what, off, units, unit_words, p, words});
  if ((int)c->trace_slots.size() - 1 == c->trace_stop) c->trace_halt = true;
}
int trace_finish(airfe_ctx* c, hipStream_t st) {
  if (c->trace_on && c->trace_overflow) {
    c->trace_overflow = false;
    return fail(c, "airfe_debug_trace: slot / unit table overflow — slots were dropped, slot indices do not name the launches of a full run");
  }
  if (c->trace_on && !c->trace_slots.empty()) {
    c->trace_off_h.clear();
    for (const auto& t : c->trace_slots) c->trace_off_h.push_back(t.off);
    c->trace_off_h.push_back(c->trace_slots.back().off + c->trace_slots.back().units);
    HIPCHK(c, hipMemcpyAsync(c->trace_off, c->trace_off_h.data(), c->trace_off_h.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    launch_trace_digest(c->trace_tab, c->trace_off, (int)c->trace_slots.size(), c->trace_dig, st);
  }
  return launch_status(c);
}
// behind every GROUP of trace slots: a trace_stop inside the group ends the forward here — lightglue_dev returns through trace_finish, what it calls hands it a 2
#define TRACE_HALT(rv) do { if (c->trace_halt) return rv; } while (0)

// (the matrix launches below return the launch status of their stage under cfg.check_launches, 0 otherwise: lightglue_dev / superglue_dev look once more at their end)
#define STAGE_RC(c) ((c)->cfg.check_launches ? launch_status(c) : 0)
#define RUN(x) do { if (x) return 1; } while (0)

int run_linear(airfe_ctx* c, const LinW& w, const uint16_t* x1, int ld1, int K1, const uint16_t* x2, int ld2, int M,
               int epi, int act, void* out, int ldo, hipStream_t st, bool trans, void* out2,
               float* x32, const float* rc, const float* rs) {
  GemmArgs g;
  g.X1 = x1; g.ld1 = ld1; g.K1 = K1; g.X2 = x2; g.ld2 = ld2;
  g.Wp = w.w; g.bias = w.b; g.M = M; g.N = w.N; g.cb_total = w.cbt;
  g.epi = epi; g.act = act; g.out = out; g.out2 = out2; g.ldo = ldo; g.x32 = x32;
  g.rot_cos = rc; g.rot_sin = rs; g.Np = c->Np; g.H = 4;
  g.small_max = c->gemm_small_max; g.g8_min = c->gemm8_min; g.gr_min = c->gemmr_min; g.gr_wgs = c->gemmr_wgs;
  { ProfScope ps(c, ST_LG_GEMM, st, 2.0 * M * w.K * w.N, (double)M * (w.K + w.N) * 2 + (double)w.K * w.N * 2); launch_gemm(c->mprec, w.K, trans, g, st); }
  return STAGE_RC(c);
}

// The attention inputs of one layer: head-major q|k (`qk`, rotary when rc != nullptr; q -> qout, k -> kout, or both roles in qout
// for the cross block's shared projection) and transposed V (`v`).  One streaming launch where kernels_gemmr.hip applies (large
// token counts), else the two linears separately — same arithmetic either way.
int run_qkv(airfe_ctx* c, const LinW& qk, const LinW& v, int M, void* qout, void* kout, const float* rc, const float* rs, hipStream_t st) {
  GemmArgs a, b;
  a.X1 = c->xb; a.ld1 = 256; a.K1 = 256; a.Wp = qk.w; a.bias = qk.b; a.M = M; a.N = qk.N; a.cb_total = qk.cbt;
  a.epi = EPI_HEADS; a.out = qout; a.out2 = kout; a.rot_cos = rc; a.rot_sin = rs; a.Np = c->Np; a.H = 4;
  b.X1 = c->xb; b.ld1 = 256; b.K1 = 256; b.Wp = v.w; b.bias = v.b; b.M = M; b.N = v.N; b.cb_total = v.cbt;
  b.epi = EPI_HEADS_T; b.out = c->vtb; b.Np = c->Np; b.H = 4;
  a.gr_wgs = b.gr_wgs = c->gemmr_wgs;
  if (c->qkv_pair && M >= c->gemmr_min && qk.K == 256 && v.K == 256 && gemmr_pair_applicable(a, b)) {
    { ProfScope ps(c, ST_LG_GEMM, st, 2.0 * M * 256.0 * (qk.N + v.N), (double)M * (256 + qk.N + v.N) * 2 + 256.0 * (qk.N + v.N) * 2); launch_gemmr_pair(c->mprec, a, b, st); }
    return STAGE_RC(c);
  }
  RUN(run_linear(c, qk, c->xb, 256, 256, nullptr, 0, M, EPI_HEADS, ACT_NONE, qout, 0, st, false, kout, nullptr, rc, rs));
  return run_linear(c, v, c->xb, 256, 256, nullptr, 0, M, EPI_HEADS_T, ACT_NONE, c->vtb, 0, st, true);
}

// out-proj + FFN + residual of block `b` as ONE kernel (kernels_lgblockf.hip; ReLU for LayerNorm + GELU where the block has no LayerNorm), which also computes the
// q | k | v projections of block `next`, the next attention's (FOLD; with rotary where next_rot); flops/bytes are the algorithmic ones
static int lg_blockf(airfe_ctx* c, const AttnBlock& b, int M, hipStream_t st, const AttnBlock* next, bool next_rot) {
  LgBlockFArgs a;
  a.relu = b.ln_g ? 0 : 1;
  const bool fr = lg_blockf_frag_weights();                   // the block kernel reads its A fragments from global memory: weights in fragment order (LinW::wf)
  a.attn = c->ob; a.xb = c->xb; a.x32 = c->x32; a.wo = fr ? b.out.wf : b.out.w; a.w1 = fr ? b.ffn0.wf : b.ffn0.w; a.w2 = fr ? b.ffn3.wf : b.ffn3.w;
  a.bo = b.out.b; a.b1 = b.ffn0.b; a.gamma = b.ln_g; a.beta = b.ln_b; a.b2 = b.ffn3.b; a.M = M;
  if (c->fold_out) { a.wo = nullptr; a.bo = nullptr; }       // the out-projection lives inside ffn0 (airfe_load.hip, make_ffn0_folded): the kernel's ffn.0 reads cat(x, attn)
  // one workgroup per CU and pass: ceil(M / T) workgroups run in rounds of 256, a round lasts ~T — take the T with the smaller product
  a.tokens_per_wg = ((M + 111) / 112 + 255) / 256 * 112 < ((M + 127) / 128 + 255) / 256 * 128 ? 112 : 128;
  // small token counts (the batch-1 calls of the SLAM loop: 800 tokens): 112-token passes would occupy 8 of the 256 CUs — 32- / 64-token passes
  // spread the same rows over 4x / 2x as many workgroups as long as that is still ONE round
  if (M <= 256 * 32) a.tokens_per_wg = 32;
  else if (M <= 256 * 64) a.tokens_per_wg = 64;
  if (c->lgb_tokens > 0) a.tokens_per_wg = c->lgb_tokens;          // airfe_tuning::lgb_tokens (measurement switch)
  a.mixed = c->lgb_tokens <= 0;                                     // the library's own choice: a second round of 6-tile passes where that balances the CUs (lgb_tokens = 112 forces uniform passes)
  a.n_cu = c->n_cu;
  // (algorithmic = what this context's packed network asks for: with the out-projection folded into ffn.0 its 2 * 256 * 256 FLOPs per token do not exist)
  double fl = 2.0 * M * ((c->fold_out ? 0.0 : 256.0 * 256) + 512.0 * 512 + 512.0 * 256), by = (double)M * (512 + 512 + 1024 + 512 + 1024) + (c->fold_out ? 786432.0 : 917504.0);
  if (next) {
    const LinW &nqk = next->qk, &nv = next->v;
    a.nqk_w = fr ? nqk.wf : nqk.w; a.nqk_b = nqk.b; a.nqk_n = nqk.N; a.nv_w = fr ? nv.wf : nv.w; a.nv_b = nv.b;
    a.rot_cos = next_rot ? c->rot_cos : nullptr; a.rot_sin = next_rot ? c->rot_sin : nullptr;
    a.q_out = c->qb; a.k_out = c->kb; a.vt_out = c->vtb; a.Np = c->Np; a.H = 4;
    fl += 2.0 * M * 256.0 * (nqk.N + nv.N);
    by += (double)M * (nqk.N + nv.N) * 2 + 256.0 * (nqk.N + nv.N) * 2;
  }
  { ProfScope ps(c, ST_LG_GEMM, st, fl, by); launch_lg_blockf(c->mprec, a, st); }
  return STAGE_RC(c);
}

// One residual block of either matcher on the 2-byte path, over S sequences of the arena.
//   own    the block's q | k | v projections are a launch of its own here, with rotary where `rot` (else the fused block before it carried them)
//   fused  what follows the attention is ONE kernel, which also carries the projections of `next` (rotary where next_rot); else separate launches: the out-projection
//          unless it is folded into ffn.0, ffn.0 (ReLU form: with ReLU), LayerNorm + GELU unless ReLU, ffn.3 added to the residual stream
//   label  names the block's trace slots, "L<li>.<label>.<stage>.<what>", one group per stage; nullptr: no trace (SuperGlue)
// A block whose projection is shared by q and k (qk.N = 256, LightGlue's cross half) has no k of its own: both roles read qb.
// Returns 0, 1 when a stage failed (cfg.check_launches), 2 when a trace_stop took effect.
static int attn_block_dev(airfe_ctx* c, const AttnBlock& b, int S, int cross, bool own, bool rot, bool fused, const AttnBlock* next, bool next_rot, size_t li,
                          const char* label, hipStream_t st) {
  const int Np = c->Np, M = S * Np;
  const int Mg = (M + 127) / 128 * 128;          // rows the matrix kernels run over (surplus rows: arena slack, see alloc_matcher_arena)
  const size_t Mw = (size_t)M * 128;             // 32-bit words of a [M][256] 2-byte buffer
  const bool own_k = b.qk.N == 512;
  auto tr = [&](const char* stage, const char* what, const void* p, size_t words, unsigned unit_words) {
    if (label && c->trace_on) trace(c, st, what, li, (std::string(label) + "." + stage).c_str(), p, words, unit_words);
  };
  auto tr_x = [&](const char* stage) {
    tr(stage, "x32", c->x32, (size_t)M * 256, 4096);
    tr(stage, "xb", c->xb, Mw, 2048);
  };
  auto tr_qkv = [&](const char* stage, bool k) {
    tr(stage, "q", c->qb, Mw, 512);
    if (k) tr(stage, "k", c->kb, Mw, 512);
    tr(stage, "vt", c->vtb, Mw, (unsigned)Np / 2);
  };
#define BLOCK_HALT do { if (label) TRACE_HALT(2); } while (0)
  if (own) {
    RUN(run_qkv(c, b.qk, b.v, Mg, c->qb, own_k ? c->kb : nullptr, rot ? c->rot_cos : nullptr, rot ? c->rot_sin : nullptr, st));
    tr_qkv("qkv", own_k);
    BLOCK_HALT;
  }
  {
    // 1 / sqrt(d_head) and log2 e are already inside q and k (ATT_QK_FOLD), so the kernel exponentiates the raw products
    ProfScope ps(c, ST_LG_ATTENTION, st, 4.0 * S * Np * (double)Np * 256, (double)M * 2048);
    launch_attention32(c->mprec, c->qb, own_k ? c->kb : c->qb, c->vtb, c->ob, c->lens, S, 4, Np, cross, st);
  }
  if (label) {          // the trace reads what the stage wrote: its launches are looked at first
    RUN(STAGE_RC(c));
    tr("attn", "o", c->ob, Mw, 2048);
    BLOCK_HALT;
  }
  if (fused) {
    RUN(lg_blockf(c, b, Mg, st, next, next_rot));
    tr_x("block");
    BLOCK_HALT;
    if (next) tr_qkv("block", next->qk.N == 512);
    BLOCK_HALT;
    return 0;
  }
  if (!c->fold_out) {
    RUN(run_linear(c, b.out, c->ob, 256, 256, nullptr, 0, Mg, EPI_STORE, ACT_NONE, c->msg, 256, st));
    tr("out", "msg", c->msg, Mw, 2048);
    BLOCK_HALT;
  }
  RUN(run_linear(c, b.ffn0, c->xb, 256, 256, c->fold_out ? c->ob : c->msg, 256, Mg, EPI_STORE, b.ln_g ? ACT_NONE : ACT_RELU, c->hb, 512, st));      // fold_out: cat(x, attention output)
  if (b.ln_g) { ProfScope ps(c, ST_LG_LNGELU, st, 0, (double)Mg * 2048); launch_ln_gelu(c->mprec, c->hb, b.ln_g, b.ln_b, Mg, st); }
  RUN(run_linear(c, b.ffn3, c->hb, 512, 512, nullptr, 0, Mg, EPI_RESID, ACT_NONE, c->xb, 256, st, false, nullptr, c->x32));
  tr_x("ffn");
  BLOCK_HALT;
  return 0;
#undef BLOCK_HALT
}

// The surplus rows behind the last real token (alloc_matcher_arena's slack) go through every block like real ones: their residual
// stream would keep growing from step to step (x += f(x), never re-initialised) until the 2-byte shadow overflows — and the last
// sequence's final key tile multiplies those rows' V by probability 0, which is NaN once they are not finite.  Back to zero per call.
void reset_slack_rows(airfe_ctx* c, int M, hipStream_t st) {
  if ((size_t)M >= c->arena_rows) return;
  launch_zero16(c->x32 + (size_t)M * 256, (c->arena_rows - (size_t)M) * 256 * sizeof(float), st);
  launch_zero16(c->xb + (size_t)M * 256, (c->arena_rows - (size_t)M) * 256 * sizeof(uint16_t), st);
}

// SuperGlue's front for production and airfe_debug_sg_front: x = descriptor + keypoint encoder; split: its two large layers (98 of 108 kFLOP per keypoint) as MFMA GEMMs
int sg_front_dev(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int normalize, bool split, hipStream_t st) {
  const int Np = c->Np, M = 2 * B * Np, Mg = (M + 127) / 128 * 128;
  const KpNorm k = kp_norm(c, 0.7f);
  reset_slack_rows(c, M, st);
  launch_sg_prepare(c->mprec == 2 ? 1 : c->mprec, f0, f1, n0, n1, AIRFE_FEAT_DIM, normalize, k.cx, k.cy, k.linv, c->sg_kenc, B, cap, Np, c->x32, c->xb, c->lens, split ? c->msg : nullptr, st);
  if (split && Mg > M) {          // the surplus rows of the 128-row rounding: zero inputs, so that the residual add leaves x = b4-ish garbage, not a running sum
    HIPCHK(c, hipMemsetAsync(c->msg + (size_t)M * 128, 0, (size_t)(Mg - M) * 128 * 2, st));
    HIPCHK(c, hipMemsetAsync(c->x32 + (size_t)M * 256, 0, (size_t)(Mg - M) * 256 * 4, st));
  }
  if (split) RUN(run_linear(c, c->sg_k3, c->msg, 128, 128, nullptr, 0, Mg, EPI_STORE, ACT_RELU, c->hb, 256, st));
  return split ? run_linear(c, c->sg_k4, c->hb, 256, 256, nullptr, 0, Mg, EPI_RESID, ACT_NONE, c->xb, 256, st, false, nullptr, c->x32) : 0;
}

// LightGlue forward on B pairs whose feature rows live on the device
int lightglue_dev(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int ld,
                  int kp_off, int normalize, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, float* scores_out,
                  hipStream_t st, const LgSecondPair* x2) {
  if (!c->has_lg) return fail(c, "LightGlue weights were not loaded (cfg.lightglue_pack)");
  if (B < 1 || B > c->Pmax) return fail(c, "pair batch exceeds cfg.max_batch / 2");
  if (cap > c->Np) return fail(c, "feature capacity exceeds the matcher arena (max_keypoints)");
  // (the second pair was looked at only behind the fp32 dispatch, which dropped it silently)
  if (x2 && (B != 1 || c->Pmax < 2 || c->mprec == 2)) return fail(c, "lightglue: a second pair needs B = 1, max_batch >= 2 and fp16 / bf16 (matcher_precision)");
  if (c->mprec == 2) return lightglue_dev_f32(c, f0, n0, f1, n1, B, cap, ld, kp_off, normalize, d_idx, d_score, mcap, d_nmatch, scores_out, st);
  LgPrepArgs pa = lg_prep_args(c, f0, n0, f1, n1, B, cap, ld, kp_off, normalize);
  if (x2) {                                      // the stereo and the temporal pair of one keyframe as a batch of two
    pa.f0x = x2->f0; pa.f1x = x2->f1; pa.n0x = x2->n0; pa.n1x = x2->n1;
    B = 2;
  }
  const int S = 2 * B, Np = c->Np, M = S * Np;
  const int Mg = (M + 127) / 128 * 128;          // rows the matrix kernels run over (surplus rows: arena slack, see alloc_matcher_arena)
  // the arena's slack rows go back to zero with the same launch (see reset_slack_rows; ADVICE r03: this line had moved to the fp32
  // path only, so that the 2-byte path's slack rows kept their running residual from call to call)
  // (only the rows a kernel of THIS call can touch: the 112- / 128-row rounding of the matrix kernels + one key tile)
  pa.slack_rows = (int)std::min(c->arena_rows - (size_t)M, (size_t)512);
  if (c->trace_on) { c->trace_slots.clear(); c->trace_overflow = false; }
  c->trace_halt = false;
  const size_t Mw = (size_t)M * 128;                     // 32-bit words of a [M][256] 2-byte buffer
  { ProfScope ps(c, ST_LG_PREPARE, st, 0, (double)M * (1036 + 1536 + 256)); launch_lg_prepare(c->mprec, pa, st); }
  trace(c, st, "x32", 0, "prep", c->x32, (size_t)M * 256, 4096);
  trace(c, st, "xb", 0, "prep", c->xb, Mw, 2048);
  // the arena's slack rows as this call starts (must be zero: ADVICE r03 / test_slack_rows_are_reset_on_every_call) and, at the end, as it leaves them
  const size_t slack_words = (size_t)(pa.slack_rows / 16 * 16) * 256;
  if (slack_words) trace(c, st, "x32slack", 0, "prep", c->x32 + (size_t)M * 256, slack_words, 4096);
  trace(c, st, "rc", 0, "prep", c->rot_cos, (size_t)M * 32, 512);
  trace(c, st, "rs", 0, "prep", c->rot_sin, (size_t)M * 32, 512);
  TRACE_HALT(trace_finish(c, st));
  // The fused block (kernels_lgblockf.hip) streams 0.9 MB of weights per workgroup whatever the batch: with 112- / 128-token passes only, the four
  // separate launches were quicker below 3200 tokens (profiles/r01d_small_batch_sweeps.txt); with 32- / 64-token passes for small token counts
  // (lg_blockf() picks them) the fused form wins everywhere (profiles/r04_lg_small_batch_sweep.txt) and block_min is 0.
  const bool fused_block = c->fuse_lg_block == 1 || (c->fuse_lg_block < 0 && Mg >= c->block_min);
  // With the fused block the projections of the NEXT attention are computed inside it (FOLD): only the very first q | k | v projection is a launch of its own.
  const bool fold = fused_block && c->fold_qkv;
  // 2 L half-steps, self (rotary; q, k and v) and cross (one shared projection for q and k: the two sides swap roles) alternating
  const size_t H = 2 * c->lg.size();
  auto half = [&](size_t h) -> const AttnBlock& { return h & 1 ? c->lg[h / 2].cross : c->lg[h / 2].self; };
  for (size_t h = 0; h < H; ++h) {
    const bool cross = h & 1, carry = fold && h + 1 < H;      // (what a cross half carries is a self half's: with rotary)
    const int rc = attn_block_dev(c, half(h), S, cross, !fold || h == 0, !cross, fused_block, carry ? &half(h + 1) : nullptr, cross, h / 2, cross ? "cross" : "self", st);
    if (rc) return rc == 2 ? trace_finish(c, st) : 1;
  }
  const size_t LF = c->lg.size();
  RUN(run_linear(c, c->lg_final, c->xb, 256, 256, nullptr, 0, Mg, EPI_STORE, ACT_NONE, c->mdb, 256, st));
  trace(c, st, "md", LF, "final", c->mdb, Mw, 2048);
  if (slack_words) trace(c, st, "x32slack", LF, "final", c->x32 + (size_t)M * 256, slack_words, 4096);
  TRACE_HALT(trace_finish(c, st));
  // the assignment tail in a scope of its own: its stage's launch status is noted before trace_finish looks at it
  const bool fused_assign = c->assign_fused == 1;      // (measured both ways on one box: profiles/r05_assign_ab.txt; ONE form for every batch size: a pair's bits do not depend on the batch)
  const int tail = [&]() -> int {
    // algorithmic: the similarity product (fused form: twice) and, round-2 form, the matrix written once and read four times / fused form, the descriptors + partials
    ProfScope ps(c, ST_LG_ASSIGN, st, (fused_assign ? 4.0 : 2.0) * B * Np * (double)Np * 256,
                 fused_assign ? (double)B * Np * (2.0 * 512 + 4.0 * 8 * ((Np + 63) / 64)) : (double)B * Np * Np * 4 * 6);
    launch_rowdot256(c->x32, c->lg_mw, c->lg_mb, c->zbuf, M, st);
    trace(c, st, "z", LF, "final", c->zbuf, (size_t)M, 16);
    TRACE_HALT(2);
    if (fused_assign) {           // no similarity matrix in HBM: log-sum-exp and arg-max partials are taken in the similarity tiles (kernels_lg.hip)
      launch_lg_assign_fused(c->mprec, c->mdb, c->zbuf, c->lens, B, Np, mcap, 0.1f, c->lg_part, c->lg_argpart, c->rowlse, c->collse,
                             c->trace_on ? c->simbuf : nullptr, scores_out, c->rowarg, c->rowval, c->colarg, d_idx, d_score, d_nmatch, st);
    } else {
      launch_sim(c->mprec, c->mdb, c->simbuf, B, Np, st);
    }
    trace(c, st, "sim", LF, "final", c->simbuf, (size_t)B * Np * Np, 16u * (unsigned)Np);
    TRACE_HALT(2);
    if (!fused_assign)
      launch_lg_assign(c->simbuf, c->zbuf, c->lens, B, Np, mcap, 0.1f, c->rowlse, c->collse, scores_out, c->rowarg, c->rowval,
                       c->colarg, d_idx, d_score, d_nmatch, st);
    auto tr_assign = [&](const char* what, const void* p) { trace(c, st, what, LF, "assign", p, (size_t)B * Np, (unsigned)Np); };
    tr_assign("rowlse", c->rowlse);
    TRACE_HALT(2);
    tr_assign("collse", c->collse);
    TRACE_HALT(2);
    tr_assign("rowval", c->rowval);
    TRACE_HALT(2);
    tr_assign("rowarg", c->rowarg);
    TRACE_HALT(2);
    tr_assign("colarg", c->colarg);
    return 0;
  }();
  (void)tail;
  return trace_finish(c, st);
}

// SuperGlue forward on B pairs of device feature matrices (259-float rows) -> decode outputs [B][Lz]
int superglue_dev(airfe_ctx* c, const float* f0, const int* n0, const float* f1, const int* n1, int B, int cap, int normalize,
                  hipStream_t st) {
  if (!c->has_sg) return fail(c, "SuperGlue weights were not loaded (cfg.superglue_pack)");
  if (B < 1 || B > c->Pmax) return fail(c, "pair batch exceeds cfg.max_batch");
  if (cap > c->Np) return fail(c, "feature capacity exceeds the matcher arena (max_keypoints)");
  if (c->mprec == 2) return superglue_dev_f32(c, f0, n0, f1, n1, B, cap, normalize, st);
  const int S = 2 * B, Np = c->Np, M = S * Np;
  const int Mg = (M + 127) / 128 * 128;
  RUN(sg_front_dev(c, f0, n0, f1, n1, B, cap, normalize, c->sg_kenc_gemm == 1 || (c->sg_kenc_gemm < 0 && Mg >= c->block_min), st));      // split from block_min tokens on
  const bool fused_block = c->fuse_lg_block == 1 || (c->fuse_lg_block < 0 && Mg >= c->block_min);
  int li = 0;      // names = ['self', 'cross'] * 9; every layer launches its own projections (no rotary), nothing is traced
  for (const AttnBlock& l : c->sg) RUN(attn_block_dev(c, l, S, li++ & 1, true, false, fused_block, nullptr, false, 0, nullptr, st));
  RUN(run_linear(c, c->sg_final, c->xb, 256, 256, nullptr, 0, Mg, EPI_STORE, ACT_NONE, c->mdb, 256, st));
  launch_sim(c->mprec, c->mdb, c->simbuf, B, Np, st);
  sg_transport_dev(c, B, st);
  return launch_status(c);
}

// The register-resident Sinkhorn kernel raises a device word when one of its bounded rendezvous spins timed out (that pair's Z is NaN): read
// after a synchronisation, cleared once reported.
int sinkhorn_failed(airfe_ctx* c) {
  if (!c->has_sg || !c->sg_cnt) return 0;
  unsigned f = 0;
  unsigned* flag = c->sg_cnt + (size_t)c->Pmax * 16;
  if (hipMemcpy(&f, flag, 4, hipMemcpyDeviceToHost) != hipSuccess || f == 0) return 0;
  (void)hipMemset(flag, 0, 4);
  return fail(c, "SuperGlue: a Sinkhorn rendezvous timed out (workgroups of the cooperative launch not co-resident?): the scores of that call are NaN");
}

}  // namespace airfe_host

extern "C" {

static int lg_host(airfe_ctx* c, const float* f0, int n0, const float* f1, int n1, int32_t* idx, float* score, int cap,
                   int* nmatch, float* scores_full) {
  AIRFE_ENTER(c);
  if (n0 < 1 || n1 < 1) { if (nmatch) *nmatch = 0; return 0; }   // point_matcher.cc:53-55
  if (n0 > c->cfg.max_keypoints || n1 > c->cfg.max_keypoints) return fail(c, "keypoint count exceeds max_keypoints");
  // ONE H2D: [n0 n1 | n0 rows of f0 | n1 rows of f1] assembled in the pinned block (f1 sits right behind f0's rows on the device too)
  const size_t b0 = (size_t)n0 * 258 * 4, b1 = (size_t)n1 * 258 * 4;
  if (ensure_pin(c, 64 + b0 + b1)) return 1;
  reinterpret_cast<int*>(c->pin)[0] = n0;
  reinterpret_cast<int*>(c->pin)[1] = n1;
  memcpy(c->pin + 64, f0, b0);
  memcpy(c->pin + 64 + b0, f1, b1);
  HIPCHK(c, hipMemcpyAsync(c->io_in, c->pin, 64 + b0 + b1, hipMemcpyHostToDevice, c->stream));
  const float* d_f1 = c->st_feat0 + (size_t)n0 * 258;
  if (lightglue_dev(c, c->st_feat0, c->st_n0, d_f1, c->st_n1, 1, c->Np, 258, 0, 0, c->st_idx, c->st_score, c->Np,
                    c->st_nm, scores_full ? c->st_scores_full : nullptr, c->stream))
    return 1;
  // ONE D2H: [nmatch | idx | score] (a few KB whatever the count), the rows copied out after the synchronisation
  const size_t ob = 64 + (size_t)c->Np * 12;
  HIPCHK(c, hipMemcpyAsync(c->pin, c->io_out, ob, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int nm = *reinterpret_cast<const int*>(c->pin);
  if (idx && score) {
    nm = std::min(nm, cap);
    matches_out(c, 64, (size_t)c->Np * 8, 0, nm, idx, score);
  }
  if (nmatch) *nmatch = nm;
  if (scores_full)
    for (int i = 0; i < n0; ++i)
      HIPCHK(c, hipMemcpy(scores_full + (size_t)i * n1, c->st_scores_full + (size_t)i * c->Np, (size_t)n1 * 4, hipMemcpyDeviceToHost));
  return 0;
}

int airfe_match_lightglue(airfe_ctx* c, const float* f0, int n0, const float* f1, int n1, int32_t* idx, float* score,
                          int cap, int* nmatch) try {
  if (c && enter_device(c)) return 1;
  return lg_host(c, f0, n0, f1, n1, idx, score, cap, nmatch, nullptr);
} AIRFE_CATCH(c)

int airfe_debug_lightglue_scores(airfe_ctx* c, const float* f0, int n0, const float* f1, int n1, float* scores) try {
  if (c && enter_device(c)) return 1;
  return lg_host(c, f0, n0, f1, n1, nullptr, nullptr, 0, nullptr, scores);
} AIRFE_CATCH(c)

int airfe_match_lightglue_batch_dev(airfe_ctx* c, const float* d_f0, const int* d_n0, const float* d_f1, const int* d_n1,
                                    int B, int cap, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, void* stream) try {
  AIRFE_ENTER(c);
  return lightglue_dev(c, d_f0, d_n0, d_f1, d_n1, B, cap, AIRFE_FEAT_DIM, 1, 1, d_idx, d_score, mcap, d_nmatch, nullptr,
                       stream_of(c, stream));
} AIRFE_CATCH(c)

static int sg_host(airfe_ctx* c, const float* f0, int n0, const float* f1, int n1, int32_t* idx0, int32_t* idx1, double* ms0,
                   double* ms1, float* scores_full) {
  AIRFE_ENTER(c);
  if (n0 < 1 || n1 < 1) return fail(c, "airfe_match_superglue: empty input (MatchingPoints early-outs before calling infer)");
  if (n0 > c->cfg.max_keypoints || n1 > c->cfg.max_keypoints) return fail(c, "keypoint count exceeds max_keypoints");
  HIPCHK(c, hipMemcpyAsync(c->st_feat0, f0, (size_t)n0 * 259 * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->st_feat1, f1, (size_t)n1 * 259 * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->st_n0, &n0, 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->st_n1, &n1, 4, hipMemcpyHostToDevice, c->stream));
  if (superglue_dev(c, c->st_feat0, c->st_n0, c->st_feat1, c->st_n1, 1, c->Np, 0, c->stream)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (sinkhorn_failed(c)) return 1;
  if (idx0) {
    std::vector<float> m0(n0), m1(n1);
    HIPCHK(c, hipMemcpy(idx0, c->sg_out0, (size_t)n0 * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(idx1, c->sg_out1, (size_t)n1 * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(m0.data(), c->sg_ms0, (size_t)n0 * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(m1.data(), c->sg_ms1, (size_t)n1 * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n0; ++i) ms0[i] = (double)m0[i];      // VectorXd filled from float vectors: super_glue.cpp:464-469
    for (int j = 0; j < n1; ++j) ms1[j] = (double)m1[j];
  }
  if (scores_full)
    HIPCHK(c, hipMemcpy2D(scores_full, (size_t)(n1 + 1) * 4, c->sg_Z, (size_t)c->Lz * 4, (size_t)(n1 + 1) * 4, n0 + 1, hipMemcpyDeviceToHost));
  return 0;
}

int airfe_match_superglue(airfe_ctx* c, const float* f0, int n0, const float* f1, int n1, int32_t* idx0, int32_t* idx1,
                          double* ms0, double* ms1) try {
  if (c && enter_device(c)) return 1;
  return sg_host(c, f0, n0, f1, n1, idx0, idx1, ms0, ms1, nullptr);
} AIRFE_CATCH(c)

/* SuperGlue on B pairs of DEVICE feature matrices (259-float rows, original pixel coordinates; NormalizeKeypoints with scale 0.7 on
   the device): d_idx0 / d_idx1 [B][cap] (-1 = unmatched), d_ms0 / d_ms1 [B][cap] floats.  No reference counterpart (batch-1 there). */
int airfe_match_superglue_batch_dev(airfe_ctx* c, const float* d_f0, const int* d_n0, const float* d_f1, const int* d_n1, int B, int cap,
                                    int32_t* d_idx0, int32_t* d_idx1, float* d_ms0, float* d_ms1, void* stream) try {
  AIRFE_ENTER(c);
  hipStream_t st = stream_of(c, stream);
  if (superglue_dev(c, d_f0, d_n0, d_f1, d_n1, B, cap, 1, st)) return 1;
  const size_t sp = (size_t)c->Lz * 4, dp = (size_t)cap * 4, wb = (size_t)std::min(cap, c->Lz) * 4;
  HIPCHK(c, hipMemcpy2DAsync(d_idx0, dp, c->sg_out0, sp, wb, B, hipMemcpyDeviceToDevice, st));
  HIPCHK(c, hipMemcpy2DAsync(d_idx1, dp, c->sg_out1, sp, wb, B, hipMemcpyDeviceToDevice, st));
  HIPCHK(c, hipMemcpy2DAsync(d_ms0, dp, c->sg_ms0, sp, wb, B, hipMemcpyDeviceToDevice, st));
  HIPCHK(c, hipMemcpy2DAsync(d_ms1, dp, c->sg_ms1, sp, wb, B, hipMemcpyDeviceToDevice, st));
  return 0;
} AIRFE_CATCH(c)

/* full SuperGlue output `scores` [n0+1][n1+1] (binding A.5) for one HOST pair */
int airfe_debug_superglue_scores(airfe_ctx* c, const float* f0, int n0, const float* f1, int n1, float* scores) try {
  if (c && enter_device(c)) return 1;
  return sg_host(c, f0, n0, f1, n1, nullptr, nullptr, nullptr, nullptr, scores);
} AIRFE_CATCH(c)

}  // extern "C"
