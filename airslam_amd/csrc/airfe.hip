// airfe — context life cycle, scratch blocks, host staging, profiling / trace, sync and status, and the two small stand-alone stages (BoW vocabulary,
// rectification) of libairfe.so's C ABI (include/airfe.h, include/airfe_debug.h).  Where the pipelines and the other entries live: airfe_host.h.
#include "airfe_host.h"

namespace airfe_host {
thread_local std::string g_err;

int fail(airfe_ctx* c, const std::string& m) {
  if (c) c->err = m;
  g_err = m;
  return 1;
}

// the catch blocks of the C boundary end here: nothing in it may throw again
int fail_noexcept(airfe_ctx* c, const char* what, const char* detail) noexcept {
  try {
    std::string m = std::string("airfe: C++ exception at the C boundary (") + what + "): " + (detail ? detail : "unknown");
    if (c) c->err = m;
    g_err = m;
  } catch (...) {
  }
  return 1;
}

int launch_status(airfe_ctx* c) {
  std::string m;
  if (c->launch_err.empty()) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    m = std::string("kernel launch failed: ") + hipGetErrorString(e);
  } else {
    m.swap(c->launch_err);
  }
  // an error path: whatever the call had queued before the failed launch (uploads from the pinned block, kernels on either stream) is drained, so that the
  // next call starts from an idle context
  (void)hipDeviceSynchronize();
  (void)hipGetLastError();
  return fail(c, m);
}

int saturation_status(airfe_ctx* c) {
  if (!c->sat_host) return 0;
  const int v0 = reinterpret_cast<volatile int*>(c->sat_host)[0], v1 = reinterpret_cast<volatile int*>(c->sat_host)[1];
  if (!v0 && !v1) return 0;
  c->sat_host[0] = c->sat_host[1] = 0;
  return fail(c, std::string("the detector's 2-byte activations left the ") + (c->prec == 1 ? "fp16" : "bf16") + " range (" + (v0 ? "non-finite score logits" : "") +
                     (v0 && v1 ? ", " : "") + (v1 ? "non-finite descriptors" : "") +
                     "): no keypoints are returned for this call.  Re-pack the detector weights with airslam_amd.weights.fold_activation_scales "
                     "(tools/onnx_to_pack.py does it: exact power-of-two rescaling between layers) or run cfg.precision = 2");
}

}  // namespace airfe_host

void note_launch(airfe_ctx* c, int stage) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess || !c->launch_err.empty()) return;
  try { c->launch_err = std::string(kStageNames[stage]) + ": kernel launch failed: " + hipGetErrorString(e); } catch (...) {}
}
namespace { __global__ void never_launched_kernel() {} }
void fail_launch_now(hipStream_t st) { hipLaunchKernelGGL(never_launched_kernel, dim3(1), dim3(4096), 0, st); }      // 4096 threads per workgroup: hipErrorInvalidConfiguration

void KfState::save(const airfe_ctx* c) {
  nms_map_valid = c->nms_map_valid; desc_normalised = c->desc_normalised; desc_dense_valid = c->desc_dense_valid; line_sparse = c->line_sparse; last_B = c->last_B;
}
void KfState::restore(airfe_ctx* c) const {
  c->nms_map_valid = nms_map_valid; c->desc_normalised = desc_normalised; c->desc_dense_valid = desc_dense_valid; c->line_sparse = line_sparse; c->last_B = last_B;
}

void release(airfe_ctx* c, DevBlock& b) {
  if (b.p) {
    auto it = std::find(c->allocs.begin(), c->allocs.end(), (void*)b.p);
    if (it != c->allocs.end()) c->allocs.erase(it);
    (void)hipFree(b.p);
  }
  b = DevBlock{};
}

int reserve(airfe_ctx* c, DevBlock& b, size_t bytes, hipStream_t st) {
  if (bytes > b.bytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (b.last && b.last != c->stream) HIPCHK(c, hipStreamSynchronize(b.last));
    c->allocs.push_back(nullptr);      // the slot first (nothing below throws: the new block is never lost between hipMalloc and the list)
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) c->allocs.pop_back();
    HIPCHK(c, e);
    release(c, b);                     // erases the old block's entry; the new slot stays the last
    c->allocs.back() = p;
    b.p = reinterpret_cast<uint8_t*>(p);
    b.bytes = bytes;
  }
  b.last = st;
  return 0;
}

// the pinned host block (grows by replacement; the stream is idle whenever a host entry starts: they all end with a synchronisation)
int ensure_pin(airfe_ctx* c, size_t bytes) {
  if (bytes <= c->pin_bytes) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint8_t* p = nullptr;
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault));
  if (c->pin) (void)hipHostFree(c->pin);
  c->pin = p;
  c->pin_bytes = bytes;
  return 0;
}

// host image -> c->st_img with the SAME row pitch: exactly (h - 1) * stride + w bytes are read (a cv::Mat ROI / numpy view has no
// bytes behind its last row's w-th pixel that are ours to read)
int upload_image(airfe_ctx* c, const uint8_t* gray, int h, int w, int stride) {
  if (!gray || h < 1 || w < 1) return fail(c, "empty image");     // plnet.cpp:247
  if (stride < w) return fail(c, "image stride smaller than its width");
  const size_t bytes = (size_t)(h - 1) * stride + w;
  if (reserve(c, c->st_img, (size_t)h * stride, c->stream)) return 1;
  // through the pinned block: a pageable hipMemcpyAsync is staged by the runtime in chunks, synchronously (measured: 2.4x the time)
  if (ensure_pin(c, bytes)) return 1;
  clear_saturation(c);
  memcpy(c->pin, gray, bytes);
  HIPCHK(c, hipMemcpyAsync(c->st_img.p, c->pin, bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// ================================================================================== C ABI
extern "C" {

void airfe_default_cfg(airfe_cfg* cfg) {
  memset(cfg, 0, sizeof(*cfg));
  cfg->device = 0;
  cfg->precision = 1;              // fp16 storage: what the reference builds its engines with (super_point.cpp:97, plnet.cpp:216)
  cfg->max_batch = 2;
  cfg->enc_chunk = 64;   // measured: per-launch fixed costs dominate below ~16 images (16: -3 %, 32: -1.7 % against 64, 128: +1.7 % on the conv64 stage); no Infinity-Cache benefit from small chunks
  cfg->max_keypoints = 400;        // configs/visual_odometry/vo_euroc.yaml:3-5
  cfg->keypoint_threshold = 0.004f;
  cfg->remove_borders = 4;
  cfg->nms_radius = 4;
  cfg->line_threshold = 0.75f;
  cfg->line_length_threshold = 50.f;
  cfg->matcher = 0;
  cfg->image_width = 752;
  cfg->image_height = 480;
  cfg->sinkhorn_iters = 100;
  cfg->matcher_precision = 1;      // fp16, what the reference builds its matcher engines with (light_glue.cpp:115, super_glue.cpp:132)
  cfg->line_precision = 0;         // stage 1: fp32 operands as fp16 (hi, lo) pairs on the 2-byte matrix pipe; f32-input MFMA in fp32 mode (include/airfe.h)
  cfg->check_launches = 0;
  cfg->tuning = nullptr;
}

void airfe_default_tuning(airfe_tuning* t) {
  if (!t) return;
  int* p = reinterpret_cast<int*>(t);
  for (size_t i = 0; i < sizeof(*t) / sizeof(int); ++i) p[i] = -1;
}

const char* airfe_last_error(const airfe_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int airfe_create(const airfe_cfg* cfg, airfe_ctx** out) try {
  if (!cfg || !out) return fail(nullptr, "airfe_create: null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(nullptr, "airfe_create: no HIP device visible (the product path has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, "airfe_create: bad device ordinal");
  if (cfg->max_keypoints < 1 || cfg->max_keypoints > 1024) return fail(nullptr, "airfe_create: max_keypoints must be 1..1024");
  if (cfg->precision < 0 || cfg->precision > 2) return fail(nullptr, "airfe_create: precision must be 0 (bf16), 1 (fp16) or 2 (fp32)");
  if (cfg->matcher_precision < -1 || cfg->matcher_precision > 2)
    return fail(nullptr, "airfe_create: matcher_precision must be -1 (= precision), 0 (bf16), 1 (fp16) or 2 (fp32)");
  if (hipSetDevice(cfg->device) != hipSuccess) return fail(nullptr, "airfe_create: hipSetDevice failed");
  // (owned by a guard until the very end: an exception below — a weight pack that does not fit the host's memory, say — must not leak the arena)
  struct Guard { airfe_ctx* p; ~Guard() { if (p) airfe_destroy(p); } } guard{new airfe_ctx()};
  airfe_ctx* c = guard.p;
  c->cfg = *cfg;
  c->prec = cfg->precision;
  c->mprec = cfg->matcher_precision < 0 ? cfg->precision : cfg->matcher_precision;
  c->pack_prec = c->prec;
  if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess) c->n_cu = 0;
  c->Bmax = std::max(cfg->max_batch, 1);
  c->chunk = std::min(std::max(cfg->enc_chunk, 1), c->Bmax);
  c->Pmax = c->Bmax;
  c->Np = (cfg->max_keypoints + 15) / 16 * 16;      // matcher rows per sequence: whole 16-token MFMA tiles, no further padding
  if (cfg->line_precision < 0 || cfg->line_precision > 3) { return fail(nullptr, "airfe_create: line_precision must be 2 (fp32 operands, f32-input MFMA) or 3 (fp32 operands as fp16 pairs on the 2-byte MFMA)"); }
  if (c->cfg.line_precision == 0) c->cfg.line_precision = c->prec == 2 ? 2 : 3;      // fp32 mode: every product of the path on f32 operands
  if (c->cfg.line_precision == 1)
    return fail(nullptr, "airfe_create: line_precision = 1 (plain fp16 operands in PLNet stage 1) is refused: measured with the real weights it moves 0.5-0.9 % of the kept "
                         "lines across the 0.75 threshold (profiles/r05_s1_fp16_emulation.txt); line_precision = 3 runs the same products on the 2-byte matrix pipe "
                         "with fp16 (hi, lo) operand pairs and keeps the lines");
  c->cfg.tuning = nullptr;                       // (the caller's struct need not outlive this call)
  if (const airfe_tuning* t = cfg->tuning) {     // kernel-selection overrides: -1 = keep the default
    for (int r : t->reserved)
      if (r != -1) { return fail(nullptr, "airfe_create: airfe_tuning.reserved must be -1 (use airfe_default_tuning)"); }
    if (t->fuse_lg_block >= 0) c->fuse_lg_block = t->fuse_lg_block != 0;
    if (t->gemm_small_max_m >= 0) c->gemm_small_max = t->gemm_small_max_m;
    if (t->gemm8_min_m >= 0) c->gemm8_min = t->gemm8_min_m;
    if (t->gemmr_min_m >= 0) c->gemmr_min = t->gemmr_min_m;
    if (t->gemmr_wgs >= 0) c->gemmr_wgs = t->gemmr_wgs;
    if (t->qkv_pair >= 0) c->qkv_pair = t->qkv_pair != 0;
    if (t->block_min_m >= 0) c->block_min = t->block_min_m;
    if (t->lgb_tokens >= 0) {
      if (t->lgb_tokens != 32 && t->lgb_tokens != 64 && t->lgb_tokens != 112 && t->lgb_tokens != 128) { return fail(nullptr, "airfe_create: tuning.lgb_tokens must be 32, 64, 112 or 128"); }
      c->lgb_tokens = t->lgb_tokens;
    }
    if (t->sg_kenc_gemm >= 0) c->sg_kenc_gemm = t->sg_kenc_gemm != 0;
    if (t->fold_qkv >= 0) c->fold_qkv = t->fold_qkv != 0;
    if (t->overlap_lines >= 0) c->overlap_lines = t->overlap_lines != 0;
    if (t->kf_graph >= 0) c->kf_graph_on = t->kf_graph != 0;
    if (t->kf_spec_rows >= 0) c->kf_spec_lines = c->kf_spec_juncs = std::max(t->kf_spec_rows, 1);   // (tests: force the second round trip)
    if (t->fuse_dec >= 0) c->fuse_dec = t->fuse_dec != 0;
    if (t->assign_fused >= 0) c->assign_fused = t->assign_fused != 0 ? 1 : 0;
    if (t->fold_out_proj >= 0) c->fold_out = t->fold_out_proj != 0;
    if (t->desc_gather_stream >= 0) c->desc_gather_stream = t->desc_gather_stream != 0;
    if (t->copy_wgs > 0) c->copy_wgs = t->copy_wgs;
  }
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_feat, hipEventDisableTiming) != hipSuccess)
    return fail(nullptr, "airfe_create: stream creation failed");      // (the guard's airfe_destroy releases whatever was created)
  // a context with a detector AND the stereo matcher runs airfe_stereo_batch_dev over left + right images as one detector batch
  c->Dmax = (c->prec != 2 && cfg->superpoint_pack && cfg->lightglue_pack) ? 2 * c->Bmax : c->Bmax;
  c->chunk = std::min(std::max(cfg->enc_chunk, 1), c->Dmax);   // (a stereo step's 2 B images may go through the first layers as ONE chunk)
  c->Lmax = c->Dmax;
  int rc = 0;
  if (cfg->superpoint_pack) rc = load_superpoint(c, cfg->superpoint_pack);
  if (!rc && cfg->lightglue_pack) rc = load_lightglue(c, cfg->lightglue_pack);
  if (!rc && cfg->superglue_pack) rc = load_superglue(c, cfg->superglue_pack);
  if (!rc && cfg->plnet_s1_pack) rc = load_plnet_s1(c, cfg->plnet_s1_pack);
  if (!rc) {
    const size_t capf = (size_t)c->Np * AIRFE_FEAT_DIM;
    if (hipHostMalloc(reinterpret_cast<void**>(&c->sat_host), 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&c->sat_flag), c->sat_host, 0) != hipSuccess)
      c->sat_flag = nullptr;
    else
      memset(c->sat_host, 0, 64);
    c->io_in = dalloc<uint8_t>(c, 64 + 2 * capf * 4);
    c->io_out = dalloc<uint8_t>(c, 64 + (size_t)c->Np * 12);
    if (!c->io_in || !c->io_out || !c->sat_flag) rc = fail(c, "device allocation failed (staging)");
    else {
      c->st_n0 = reinterpret_cast<int*>(c->io_in);
      c->st_n1 = c->st_n0 + 1;
      c->st_feat0 = reinterpret_cast<float*>(c->io_in + 64);
      c->st_feat1 = c->st_feat0 + capf;
      c->st_nm = reinterpret_cast<int*>(c->io_out);
      c->st_idx = reinterpret_cast<int32_t*>(c->io_out + 64);
      c->st_score = reinterpret_cast<float*>(c->io_out + 64 + (size_t)c->Np * 8);
      if (hipHostMalloc(reinterpret_cast<void**>(&c->pin), 64 + 2 * capf * 4, hipHostMallocDefault) != hipSuccess) rc = fail(c, "hipHostMalloc failed (staging)");
      else c->pin_bytes = 64 + 2 * capf * 4;
    }
  }
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(c, "device error during weight upload");
  if (rc) {
    g_err = c->err;
    return rc;
  }
  guard.p = nullptr;
  *out = c;
  return 0;
} AIRFE_CATCH(nullptr)

void airfe_destroy(airfe_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  (void)hipDeviceSynchronize();
  c->kf_graph.reset();
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->pin) (void)hipHostFree(c->pin);
  if (c->sat_host) (void)hipHostFree(c->sat_host);
  if (c->copy_ring) (void)hipHostFree(c->copy_ring);
  for (auto& m : c->marks) { (void)hipEventDestroy(m.a); (void)hipEventDestroy(m.b); }
  for (auto e : c->ev_pool) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_feat) (void)hipEventDestroy(c->ev_feat);
  delete c;
}

int airfe_profile_enable(airfe_ctx* c, int on) try {
  AIRFE_ENTER(c);
  HIPCHK(c, hipDeviceSynchronize());             // the events may have been recorded on a caller's stream (the *_dev entry points)
  for (auto& m : c->marks) { c->ev_pool.push_back(m.a); c->ev_pool.push_back(m.b); }
  c->marks.clear();
  c->prof_mask = on < 0 ? 0xFFFFFFFFu : (uint32_t)on;
  return 0;
} AIRFE_CATCH(c)

int airfe_profile_stages(void) { return ST_COUNT; }
const char* airfe_profile_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }

int airfe_profile_read(airfe_ctx* c, double* ms, double* flops, double* bytes, int* launches) try {
  AIRFE_ENTER(c);
  HIPCHK(c, hipDeviceSynchronize());
  for (int i = 0; i < ST_COUNT; ++i) { ms[i] = 0; flops[i] = 0; bytes[i] = 0; launches[i] = 0; }
  for (auto& m : c->marks) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, m.a, m.b) == hipSuccess) {
      ms[m.stage] += t; flops[m.stage] += m.flops; bytes[m.stage] += m.bytes; launches[m.stage] += 1;
    }
    c->ev_pool.push_back(m.a); c->ev_pool.push_back(m.b);
  }
  c->marks.clear();
  return 0;
} AIRFE_CATCH(c)

/* fault hunting: checksums of the matcher's state behind every launch of the LightGlue forward (x32, xb, q, k, v^T, attention output, ...)
   in units of 16 token rows; off by default.  airfe_debug_trace_read synchronises the context's stream. */
int airfe_debug_trace(airfe_ctx* c, int on) try {
  AIRFE_ENTER(c);
  if (on && !c->trace_tab) {
    c->trace_cap = (size_t)3 << 20;
    c->trace_tab = dalloc<unsigned long long>(c, c->trace_cap);
    c->trace_dig = dalloc<unsigned long long>(c, 1024);
    c->trace_off = dalloc<unsigned>(c, 1025);
    if (!c->trace_tab || !c->trace_dig || !c->trace_off) return fail(c, "device allocation failed (trace)");
  }
  c->trace_on = on != 0;
  c->trace_slots.clear();
  return 0;
} AIRFE_CATCH(c)
int airfe_debug_trace_stop(airfe_ctx* c, int slot) try {
  AIRFE_ENTER(c);
  c->trace_stop = slot;
  return 0;
} AIRFE_CATCH(c)
int airfe_debug_trace_buffer(airfe_ctx* c, int slot, void* host, size_t bytes) try {
  if (c && enter_device(c)) return 1;
  if (!c || slot < 0 || slot >= (int)c->trace_slots.size()) return fail(c, "trace_buffer: no such slot");
  const auto& t = c->trace_slots[(size_t)slot];
  if (bytes > t.words * 4) return fail(c, "trace_buffer: more bytes than the slot covers");
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(host, t.p, bytes, hipMemcpyDeviceToHost));
  return 0;
} AIRFE_CATCH(c)
int airfe_debug_trace_slots(airfe_ctx* c) { return c ? (int)c->trace_slots.size() : 0; }
int airfe_debug_trace_slot(airfe_ctx* c, int i, char* name, int name_cap, unsigned* off, unsigned* units, unsigned* unit_words) try {
  if (!c || i < 0 || i >= (int)c->trace_slots.size()) return 1;
  const auto& t = c->trace_slots[(size_t)i];
  if (name && name_cap > 0) { strncpy(name, t.name.c_str(), (size_t)name_cap - 1); name[name_cap - 1] = 0; }
  if (off) *off = t.off;
  if (units) *units = t.units;
  if (unit_words) *unit_words = t.unit_words;
  return 0;
} AIRFE_CATCH(c)
int airfe_debug_trace_read(airfe_ctx* c, void* stream, unsigned long long* digests, unsigned long long* table) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->trace_tab) return fail(c, "trace is off");
  hipStream_t st = stream_of(c, stream);
  HIPCHK(c, hipStreamSynchronize(st));
  const size_t n = c->trace_slots.size();
  if (n == 0) return 0;
  if (digests) HIPCHK(c, hipMemcpy(digests, c->trace_dig, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (table) HIPCHK(c, hipMemcpy(table, c->trace_tab, ((size_t)c->trace_slots.back().off + c->trace_slots.back().units) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
} AIRFE_CATCH(c)

int airfe_sync(airfe_ctx* c) try {
  AIRFE_ENTER(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (saturation_status(c)) return 1;                     // (the batch entry points are asynchronous: an activation overflow of an earlier call surfaces here)
  return sinkhorn_failed(c);         // (... and a Sinkhorn time-out)
} AIRFE_CATCH(c)

int airfe_superglue_status(airfe_ctx* c, void* stream) try {
  AIRFE_ENTER(c);
  HIPCHK(c, hipStreamSynchronize(stream_of(c, stream)));
  if (saturation_status(c)) return 1;
  return sinkhorn_failed(c);
} AIRFE_CATCH(c)

/* ---- BoW quantisation behind the path: Database::FrameToBow's per-feature tree descent --------------- */
int airfe_bow_load(airfe_ctx* c, const float* node_desc, const int32_t* first_child, const int32_t* n_children, const int32_t* word_id,
                   const double* weight, int n_nodes) try {
  AIRFE_ENTER(c);
  if (!node_desc || !first_child || !n_children || !word_id || !weight || n_nodes < 1) return fail(c, "bow_load: bad argument");
  for (int i = 0; i < n_nodes; ++i) {                    // the device follows these indices: validate them here, once
    if (n_children[i] < 0 || (n_children[i] > 0 && (first_child[i] <= i || first_child[i] + n_children[i] > n_nodes)))
      return fail(c, "bow_load: children must lie after their parent and inside the node table");
  }
  if (c->bow_nodes) return fail(c, "bow_load: a vocabulary is already loaded in this context");
  std::vector<float> d(node_desc, node_desc + (size_t)n_nodes * 256), w(n_nodes);
  for (int i = 0; i < n_nodes; ++i) w[i] = (float)weight[i];
  std::vector<int> fc(first_child, first_child + n_nodes), nc(n_children, n_children + n_nodes), wi(word_id, word_id + n_nodes);
  c->bow_desc = dupload(c, d); c->bow_weight = dupload(c, w);
  c->bow_first = dupload(c, fc); c->bow_nch = dupload(c, nc); c->bow_word = dupload(c, wi);
  c->bow_out = dalloc<unsigned>(c, 1024); c->bow_outw = dalloc<float>(c, 1024); c->bow_outn = dalloc<int>(c, 1024);
  c->bow_weight_h.assign(weight, weight + n_nodes);
  c->bow_weight_d = dupload(c, c->bow_weight_h);            // WordValue is a double: the BoW vector sums these, not the float copy the descent compares with 0
  if (!c->bow_weight_d) return fail(c, "bow_load: device allocation failed");
  c->bow_nwords = 0;
  for (int i = 0; i < n_nodes; ++i)
    if (n_children[i] == 0 && word_id[i] >= 0) c->bow_nwords = std::max(c->bow_nwords, word_id[i] + 1);
  if (!c->bow_desc || !c->bow_weight || !c->bow_first || !c->bow_nch || !c->bow_word || !c->bow_out || !c->bow_outw || !c->bow_outn)
    return fail(c, "device allocation failed (vocabulary)");
  c->bow_nodes = n_nodes;
  return 0;
} AIRFE_CATCH(c)

int airfe_bow_transform_dev(airfe_ctx* c, const float* d_feat, int N, uint32_t* d_word, float* d_weight, void* stream) try {
  AIRFE_ENTER(c);
  if (!c->bow_nodes) return fail(c, "bow_transform: no vocabulary loaded (airfe_bow_load)");
  if (N < 0 || (N > 0 && (!d_feat || !d_word || !d_weight))) return fail(c, "bow_transform: bad argument");
  hipStream_t st = stream_of(c, stream);
  ProfScope ps(c, ST_BOW, st, 0, (double)N * 259 * 4);
  launch_bow_transform(d_feat, AIRFE_FEAT_DIM, 3, N, c->bow_desc, c->bow_first, c->bow_nch, c->bow_word, c->bow_weight, d_word, d_weight,
                       d_weight == c->bow_outw ? c->bow_outn : nullptr, st);
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(c)

int airfe_bow_transform(airfe_ctx* c, const float* feat, int N, uint32_t* word_of_features, double* weight_of_features) try {
  AIRFE_ENTER(c);
  if (N == 0) return 0;                                  // database.cc:60
  if (N < 0 || N > c->Np || N > 1024 || !feat || !word_of_features) return fail(c, "bow_transform: bad argument / more features than max_keypoints");
  HIPCHK(c, hipMemcpyAsync(c->st_feat0, feat, (size_t)N * AIRFE_FEAT_DIM * 4, hipMemcpyHostToDevice, c->stream));
  if (airfe_bow_transform_dev(c, c->st_feat0, N, c->bow_out, c->bow_outw, c->stream)) return 1;
  std::vector<int> node(N);
  HIPCHK(c, hipMemcpyAsync(word_of_features, c->bow_out, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(node.data(), c->bow_outn, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (weight_of_features)        // WordValue is a double in the reference (3rdparty/DBoW2 BowVector.h): the leaf's own weight, not a float round trip
    for (int i = 0; i < N; ++i) weight_of_features[i] = c->bow_weight_h[(size_t)node[i]];
  return 0;
} AIRFE_CATCH(c)

/* ---- rectification in front of the path: Camera::UndistortImage, src/camera.cc:161-182 ------------- */
int airfe_set_rectify_maps(airfe_ctx* c, int side, const float* mapx, const float* mapy, int h, int w) try {
  AIRFE_ENTER(c);
  if (side < 0 || side > 1 || !mapx || !mapy || h < 1 || w < 1) return fail(c, "set_rectify_maps: bad argument");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t n = (size_t)h * w;
  for (int k = 0; k < 2; ++k) {
    if (c->rmap[side][k]) {
      auto it = std::find(c->allocs.begin(), c->allocs.end(), (void*)c->rmap[side][k]);
      if (it != c->allocs.end()) c->allocs.erase(it);
      (void)hipFree(c->rmap[side][k]);
    }
    c->rmap[side][k] = dalloc<float>(c, n, false);
    if (!c->rmap[side][k]) return fail(c, "device allocation failed (rectification maps)");
    HIPCHK(c, hipMemcpy(c->rmap[side][k], k ? mapy : mapx, n * 4, hipMemcpyHostToDevice));
  }
  c->rmap_h[side] = h;
  c->rmap_w[side] = w;
  return 0;
} AIRFE_CATCH(c)

int airfe_rectify_batch_dev(airfe_ctx* c, int side, const uint8_t* d_raw, int B, int h, int w, int stride, size_t img_stride,
                            uint8_t* d_rect, int rstride, size_t rimg_stride, void* stream) try {
  AIRFE_ENTER(c);
  if (side < 0 || side > 1 || !c->rmap[side][0]) return fail(c, "rectify: no maps set for this side (airfe_set_rectify_maps)");
  if (h != c->rmap_h[side] || w != c->rmap_w[side]) return fail(c, "rectify: image size differs from the maps'");
  if (stride < w || rstride < w) return fail(c, "rectify: stride smaller than the width");
  hipStream_t st = stream_of(c, stream);
  ProfScope ps(c, ST_RECTIFY, st, 0, (double)B * h * w * (1 + 8 + 1));          // source pixels + two float maps + rectified pixels
  launch_remap_linear(d_raw, B, h, w, stride, img_stride, c->rmap[side][0], c->rmap[side][1], d_rect, rstride, rimg_stride, st);
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(c)

int airfe_has_line_branch(const airfe_ctx* c) { return c && c->has_s0 && c->has_s1; }

}  // extern "C"
