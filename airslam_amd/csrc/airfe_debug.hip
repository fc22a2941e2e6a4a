// airfe — the kernel-level test hooks of libairfe.so (include/airfe_debug.h): host tensors -> one production launcher -> host tensors.  Every device allocation
// of a hook lives in a DbgTmp and is freed on every way out, an exception caught by AIRFE_CATCH included.
#include "airfe_host.h"

struct DbgTmp {                                  // device allocations of one hook call, freed on every way out
  airfe_ctx h;                                   // only as an allocation list holder (dalloc / dupload / make_linear)
  DbgTmp() {}
  explicit DbgTmp(int prec) { h.prec = h.pack_prec = prec; }      // the storage type make_linear packs for
  ~DbgTmp() { for (void* p : h.allocs) (void)hipFree(p); }
};

// the conv hooks' staging: NCHW fp32 -> the arena's NHWC 2-byte layout with its zero border; [cout][cin][3][3] fp32 -> the packed slabs
static std::vector<uint16_t> dbg_conv_x(const float* x, int B, int cin, int H, int W, int prec) {
  std::vector<uint16_t> xin((size_t)B * (H + 2) * (W + 2) * cin, 0);
  for (int bb = 0; bb < B; ++bb)
    for (int ci = 0; ci < cin; ++ci)
      for (int yy = 0; yy < H; ++yy)
        for (int xx = 0; xx < W; ++xx)
          xin[(((size_t)bb * (H + 2) + yy + 1) * (W + 2) + xx + 1) * cin + ci] = cvt2(x[(((size_t)bb * cin + ci) * H + yy) * W + xx], prec);
  return xin;
}
static std::vector<uint16_t> dbg_conv_slabs(const float* w, int cin, int cout, int prec) {
  const int nci = cin / 64;
  return pack_slabs(cout / 64, 9 * nci, prec, [&](int feat, int s, int k) {
    const int tap = s / nci, cc = s % nci, ci = cc * 64 + k;
    return w[((size_t)feat * cin + ci) * 9 + tap];
  });
}

extern "C" {

// ---- kernel-level test hooks ------------------------------------------------------------------------------
int airfe_debug_preprocess(airfe_ctx* c, const uint8_t* gray, int h, int w, int stride, float* out) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_sp) return fail(c, "debug_preprocess: detector not loaded");
  const size_t bytes = (size_t)h * stride;
  if (upload_image(c, gray, h, w, stride) || ensure_tables(c, h, w)) return 1;
  const int R = AIRFE_INTERNAL_SIZE;
  launch_preprocess(c->st_img.p, 1, h, w, stride, bytes, c->xtab, c->ytab, c->lut, c->img32, R, R, c->stream);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy2D(out, (size_t)R * 4, c->img32 + (R + 2) + 1, (size_t)(R + 2) * 4, (size_t)R * 4, R, hipMemcpyDeviceToHost));
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_conv3x3(airfe_ctx* c, const float* x, int B, int cin, int H, int W, const float* w, const float* b, int cout,
                        int pool, float* y) try {
  AIRFE_ENTER(c);
  if ((cin != 64 && cin != 128) || cout % 64 || W % 16 || H % 16) return fail(c, "debug_conv3x3: unsupported shape");
  const int prec = c->prec;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  const size_t ywords = (size_t)B * (Ho + 2) * (Wo + 2) * cout;
  DbgTmp t(prec);
  airfe_ctx& tmp = t.h;
  ConvArgs a;
  a.X = dupload(&tmp, dbg_conv_x(x, B, cin, H, W, prec)); a.Wp = dupload(&tmp, dbg_conv_slabs(w, cin, cout, prec));
  a.bias = dupload(&tmp, std::vector<float>(b, b + cout)); a.Y = dalloc<uint16_t>(&tmp, ywords);
  if (!a.X || !a.Wp || !a.bias || !a.Y) return fail(c, "debug_conv3x3: allocation failed");
  a.B = B; a.H = H; a.W = W; a.CIN = cin; a.COUT = cout;
  a.pool = pool; a.out_pad = 1; a.relu = 1;
  (void)hipStreamSynchronize(nullptr);       // dalloc's zero fill of Y runs on the null stream, which the context's stream does not wait for (see dbg_canary)
  launch_conv3x3(prec, a, c->stream);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<uint16_t> yo(ywords);
  HIPCHK(c, hipMemcpy(yo.data(), a.Y, ywords * 2, hipMemcpyDeviceToHost));
  for (int bb = 0; bb < B; ++bb)
    for (int co = 0; co < cout; ++co)
      for (int yy = 0; yy < Ho; ++yy)
        for (int xx = 0; xx < Wo; ++xx)
          y[(((size_t)bb * cout + co) * Ho + yy) * Wo + xx] = back2(yo[(((size_t)bb * (Ho + 2) + yy + 1) * (Wo + 2) + xx + 1) * cout + co], prec);
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_fail_next_launch(airfe_ctx* c, int stage) try {
  AIRFE_ENTER(c);
  if (stage < -1 || stage >= ST_COUNT) return fail(c, "debug_fail_next_launch: no such stage");
  c->fail_stage = stage;
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_gemm(airfe_ctx* c, const float* x, int M, int K, const float* w, const float* b, int N, int relu, float* y) try {
  AIRFE_ENTER(c);
  if (K != 128 && K != 256 && K != 512) return fail(c, "debug_gemm: K must be 128, 256 or 512");
  const int prec = c->prec, Mp = (M + 127) / 128 * 128, Np8 = (N + 7) / 8 * 8;
  std::vector<uint16_t> xin((size_t)Mp * K, 0);
  for (size_t i = 0; i < (size_t)M * K; ++i) xin[i] = cvt2(x[i], prec);
  DbgTmp t(prec);
  airfe_ctx& tmp = t.h;
  LinW lw;
  if (!make_linear(&tmp, w, b, K, N, lw)) return fail(c, "debug_gemm: allocation failed");
  uint16_t* dx = dupload(&tmp, xin);
  float* dy = dalloc<float>(&tmp, (size_t)Mp * Np8);
  int rc = 0;
  if (!dx || !dy) rc = fail(c, "debug_gemm: allocation failed");
  if (!rc) {
    GemmArgs g;
    g.X1 = dx; g.ld1 = K; g.K1 = K; g.Wp = lw.w; g.bias = lw.b; g.M = Mp; g.N = N; g.cb_total = lw.cbt;
    g.epi = EPI_STORE_F32; g.act = relu ? ACT_RELU : ACT_NONE; g.out = dy; g.ldo = Np8;
    g.small_max = c->gemm_small_max; g.g8_min = c->gemm8_min; g.gr_min = c->gemmr_min; g.gr_wgs = c->gemmr_wgs;
    (void)hipStreamSynchronize(nullptr);     // dy's zero fill (dalloc) must not land on top of the kernel's rows (see dbg_canary; seen once as zero rows in test_gemm)
    launch_gemm(prec, K, false, g, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, "debug_gemm: kernel failed");
  }
  if (!rc) {
    std::vector<float> yo((size_t)Mp * Np8);
    (void)hipMemcpy(yo.data(), dy, yo.size() * 4, hipMemcpyDeviceToHost);
    for (int m = 0; m < M; ++m)
      for (int n = 0; n < N; ++n) y[(size_t)m * N + n] = yo[(size_t)m * Np8 + n];
  }
  return rc;
} AIRFE_CATCH(c)

}  // extern "C"

// ---- the GEMM family one form at a time (include/airfe_debug.h): host tensors -> the production launchers -> host tensors
static std::vector<uint16_t> dbg_rows2(const float* x, int rows, int cols, int rows_cap, int prec) {
  std::vector<uint16_t> v((size_t)rows_cap * cols, 0);
  if (x)
    for (size_t i = 0; i < (size_t)rows * cols; ++i) v[i] = cvt2(x[i], prec);
  return v;
}
static std::vector<float> dbg_rows4(const float* x, int rows, int cols, int rows_cap) {
  std::vector<float> v((size_t)rows_cap * cols, 0.f);
  if (x) memcpy(v.data(), x, (size_t)rows * cols * sizeof(float));
  return v;
}
template <class T>
static T* dbg_canary(airfe_ctx* tmp, size_t n) {       // an output buffer whose every byte starts as 0xFF (NaN in fp32, fp16 and bf16)
  T* p = dalloc<T>(tmp, n, false);
  if (p) {
    (void)hipMemset(p, 0xFF, std::max<size_t>(n, 1) * sizeof(T));
    // the fill of device memory runs on the null stream and may return before it is done; the hooks launch on the context's NON-BLOCKING stream, which does not
    // wait for it: without this wait the fill could land on top of a fast kernel's rows (seen once as NaN rows in tests/test_gpu_linear_kernels.py)
    (void)hipStreamSynchronize(nullptr);
  }
  return p;
}
static void dbg_back2(const std::vector<uint16_t>& v, size_t n, int prec, float* out) {
  for (size_t i = 0; i < n; ++i) out[i] = back2(v[i], prec);
}

extern "C" {

int airfe_debug_conv(airfe_ctx* c, airfe_debug_conv_args* a) try {
  AIRFE_ENTER(c);
  if (!a || !a->w || !a->b || !a->y_raw) return fail(c, "debug_conv: null argument");
  const bool fused = a->img != nullptr;
  if (fused == (a->x != nullptr)) return fail(c, "debug_conv: exactly one of x (plain form) and img (fused conv1a -> conv1b) must be given");
  const int cin = a->cin, cout = a->cout, B = a->B, H = a->H, W = a->W, pool = a->pool, opad = a->out_pad, prec = c->prec;
  if (prec != 0 && prec != 1) return fail(c, "debug_conv: the context's precision must be fp16 or bf16");
  if (a->wgs < 1 || a->wgs > 256) return fail(c, "debug_conv: wgs must lie in 1 .. 256");
  if (cin != 64 && cin != 128) return fail(c, "debug_conv: cin must be 64 or 128");
  if (cout < 64 || cout % 64 || (cin == 128 && cout % 128)) return fail(c, "debug_conv: cout must be a multiple of 64 (of 128 when cin is 128)");
  if (B < 1 || H < 16 || W < 16 || H % 16 || W % 16) return fail(c, "debug_conv: B >= 1, H and W multiples of 16");
  if ((pool != 0 && pool != 1) || (opad != 0 && opad != 1) || (a->relu != 0 && a->relu != 1)) return fail(c, "debug_conv: pool, out_pad and relu are 0 or 1");
  if (pool && !opad) return fail(c, "debug_conv: a pooled layer always feeds another conv (out_pad = 1); pool with out_pad = 0 is no form of the arena");
  if (fused && (cin != 64 || cout != 64 || !pool || !opad || !a->relu || !a->w1a || !a->b1a))
    return fail(c, "debug_conv: the fused form is conv1a -> conv1b: cin = cout = 64, pool = 1, out_pad = 1, relu = 1, w1a and b1a given");
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  const size_t guard = (size_t)(Wo + 2 * opad) * cout, words = (size_t)B * (Ho + 2 * opad) * guard, total = words + 2 * guard;
  if (a->y_words != total) return fail(c, "debug_conv: y_words must be (B (Ho + 2 out_pad) + 2) (Wo + 2 out_pad) cout");
  DbgTmp t(prec);
  airfe_ctx& tmp = t.h;
  ConvArgs g;
  if (fused) {
    std::vector<float> im((size_t)B * (H + 2) * (W + 2), 0.f);
    for (int bb = 0; bb < B; ++bb)
      for (int yy = 0; yy < H; ++yy) memcpy(&im[((size_t)bb * (H + 2) + yy + 1) * (W + 2) + 1], a->img + ((size_t)bb * H + yy) * W, (size_t)W * sizeof(float));
    g.img = dupload(&tmp, im);
    g.w1a = dupload(&tmp, std::vector<float>(a->w1a, a->w1a + 64 * 9));
    g.b1a = dupload(&tmp, std::vector<float>(a->b1a, a->b1a + 64));
  } else {
    g.X = dupload(&tmp, dbg_conv_x(a->x, B, cin, H, W, prec));
  }
  g.Wp = dupload(&tmp, dbg_conv_slabs(a->w, cin, cout, prec));
  g.bias = dupload(&tmp, std::vector<float>(a->b, a->b + cout));
  uint16_t* dy = dbg_canary<uint16_t>(&tmp, total);
  if ((fused ? !g.img || !g.w1a || !g.b1a : !g.X) || !g.Wp || !g.bias || !dy) return fail(c, "debug_conv: allocation failed");
  g.Y = dy + guard;
  g.B = B; g.H = H; g.W = W; g.CIN = cin; g.COUT = cout; g.pool = pool; g.out_pad = opad; g.relu = a->relu; g.wgs = a->wgs;
  if (fused) launch_conv64r(prec, g, c->stream);         // as detect_dev2 launches the first layer
  else launch_conv3x3(prec, g, c->stream);               // production's dispatch: conv64r / conv128r, or conv3x3_kernel for relu = 0
  if (hipStreamSynchronize(c->stream) != hipSuccess || launch_status(c)) return fail(c, "debug_conv: kernel failed");
  HIPCHK(c, hipMemcpy(a->y_raw, dy, total * 2, hipMemcpyDeviceToHost));
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_linear(airfe_ctx* c, const airfe_debug_linear_args* a) try {
  AIRFE_ENTER(c);
  if (!a || !a->x1 || !a->w || !a->b || !a->out) return fail(c, "debug_linear: null argument");
  const int prec = a->prec, M = a->M, K = a->K, N = a->N, epi = a->epi, kern = a->kernel, K1 = a->x2 ? a->K1 : K;
  if ((prec != 0 && prec != 1) || M < 1 || N < 1 || (K != 128 && K != 256 && K != 512) || K1 < 32 || K1 % 32 || K1 > K || (a->x2 && K1 == K) ||
      epi < EPI_STORE || epi > EPI_SOFTMAX_D2S || kern < AIRFE_DEBUG_KERNEL_DISPATCH || kern > AIRFE_DEBUG_KERNEL_GEMMR_GATHER128 || (a->act != ACT_NONE && a->act != ACT_RELU))
    return fail(c, "debug_linear: bad argument");
  const bool trans = epi == EPI_HEADS_T, heads = epi == EPI_HEADS || trans, d2s = epi == EPI_SOFTMAX_D2S;
  if (heads && ((a->H != 4 && a->H != 0) || a->Np < 16 || a->Np % 16 || M % a->Np || (epi == EPI_HEADS ? (N != 256 && N != 512) || (N == 512 && !a->out2) : N != 256)))
    return fail(c, "debug_linear: head layouts need H = 4, M = S * Np with Np a multiple of 16, N = 256 (or 512 with out2 for EPI_HEADS)");
  if ((a->rot_cos || a->rot_sin) && (epi != EPI_HEADS || !a->rot_cos || !a->rot_sin)) return fail(c, "debug_linear: rotary is an EPI_HEADS form");
  if (epi == EPI_RESID && (!a->x32 || N % 64)) return fail(c, "debug_linear: EPI_RESID needs x32 and N a multiple of 64");
  if (d2s && (K != 256 || N != 65 || a->x2 || a->rowidx || a->act || a->d2s_hc < 1 || a->d2s_wc < 1 || M % (a->d2s_hc * a->d2s_wc) || M % 16 ||
              (kern != AIRFE_DEBUG_KERNEL_DISPATCH && kern != AIRFE_DEBUG_KERNEL_GEMM8)))
    return fail(c, "debug_linear: EPI_SOFTMAX_D2S is launch_gemm8's head kernel: K = 256, N = 65, dense rows, M = B * hc * wc, M % 16 == 0");
  if (a->rowidx) {
    if (kern != AIRFE_DEBUG_KERNEL_GEMM8 && kern != AIRFE_DEBUG_KERNEL_GEMMR_GATHER && kern != AIRFE_DEBUG_KERNEL_GEMMR_GATHER128)
      return fail(c, "debug_linear: a row gather runs in gemm8, gemmr_gather or gemmr_gather128 only");
    if (a->src_rows < 1) return fail(c, "debug_linear: rowidx needs src_rows");
    for (int r = 0; r < M; ++r)
      if (a->rowidx[r] < 0 || a->rowidx[r] >= a->src_rows) return fail(c, "debug_linear: rowidx entry outside 0 .. src_rows - 1");
  }
  static const int row_tile[7] = {128, 32, 128, 256, 32, 32, 64};
  const int Mp = d2s ? M : (M + row_tile[kern] - 1) / row_tile[kern] * row_tile[kern];
  const int xrows = a->rowidx ? a->src_rows : Mp;
  const int ldo = (epi == EPI_STORE || epi == EPI_STORE_F32) ? (N + 7) / 8 * 8 : N;
  const int Sg = heads ? (Mp + a->Np - 1) / a->Np : 0, S = heads ? M / a->Np : 0;
  DbgTmp t(prec);
  airfe_ctx& tmp = t.h;
  LinW lw;
  if (!make_linear(&tmp, a->w, a->b, K, N, lw)) return fail(c, "debug_linear: allocation failed");
  GemmArgs g;
  g.X1 = dupload(&tmp, dbg_rows2(a->x1, a->rowidx ? a->src_rows : M, K1, xrows, prec)); g.ld1 = K1; g.K1 = K1;
  if (a->x2) { g.X2 = dupload(&tmp, dbg_rows2(a->x2, M, K - K1, Mp, prec)); g.ld2 = K - K1; }
  g.Wp = lw.w; g.bias = lw.b; g.M = Mp; g.N = N; g.cb_total = lw.cbt; g.epi = epi; g.act = a->act; g.ldo = ldo; g.Np = a->Np; g.H = 4;
  g.small_max = c->gemm_small_max; g.g8_min = c->gemm8_min; g.gr_min = c->gemmr_min; g.gr_wgs = a->gr_wgs > 0 ? a->gr_wgs : c->gemmr_wgs;
  if (a->rot_cos) { g.rot_cos = dupload(&tmp, dbg_rows4(a->rot_cos, M, 32, Mp)); g.rot_sin = dupload(&tmp, dbg_rows4(a->rot_sin, M, 32, Mp)); }
  if (a->rowidx) { std::vector<int> ri(Mp, 0); memcpy(ri.data(), a->rowidx, (size_t)M * sizeof(int)); g.rowidx = dupload(&tmp, ri); }
  size_t out_elems = 0;
  if (epi == EPI_STORE || epi == EPI_RESID) out_elems = (size_t)Mp * ldo;
  else if (heads) out_elems = (size_t)Sg * 4 * a->Np * 64;
  if (epi == EPI_STORE_F32) g.out = dbg_canary<float>(&tmp, (size_t)Mp * ldo);
  else if (d2s) g.out = dbg_canary<float>(&tmp, (size_t)M * 64);
  else g.out = dbg_canary<uint16_t>(&tmp, out_elems);
  if (epi == EPI_HEADS && N == 512) g.out2 = dbg_canary<uint16_t>(&tmp, out_elems);
  if (epi == EPI_RESID) g.x32 = dupload(&tmp, dbg_rows4(a->x32, M, N, Mp));
  if (d2s) { g.d2s_hc = a->d2s_hc; g.d2s_wc = a->d2s_wc; g.flag = dalloc<int>(&tmp, 1); }
  bool ok = g.X1 && (!a->x2 || g.X2) && g.out && (!(epi == EPI_HEADS && N == 512) || g.out2) && (epi != EPI_RESID || g.x32) && (!a->rot_cos || (g.rot_cos && g.rot_sin)) &&
            (!a->rowidx || g.rowidx) && (!d2s || g.flag);
  int rc = ok ? 0 : fail(c, "debug_linear: allocation failed");
  // a forced kernel runs only where its own applicability test says yes: never a silent fall-back to another kernel
  const char* refused = nullptr;
  if (!rc) switch (kern) {
    case AIRFE_DEBUG_KERNEL_DISPATCH:
      if (d2s) launch_gemm8(prec, K, false, g, c->stream);
      else launch_gemm(prec, K, trans, g, c->stream);
      break;
    case AIRFE_DEBUG_KERNEL_SMALL:                       // launch_gemm's own row test with every other path moved out of reach
      if (d2s || a->rowidx) refused = "gemm_small";
      else { g.small_max = 1 << 30; g.g8_min = 1 << 30; g.gr_min = 1 << 30; launch_gemm(prec, K, trans, g, c->stream); }
      break;
    case AIRFE_DEBUG_KERNEL_TILED:
      if (d2s || a->rowidx || K1 % 64) refused = "gemm_kernel";
      else { g.small_max = -1; g.g8_min = 1 << 30; g.gr_min = 1 << 30; launch_gemm(prec, K, trans, g, c->stream); }
      break;
    case AIRFE_DEBUG_KERNEL_GEMM8:
      if (K1 % 64) refused = "gemm8";
      else launch_gemm8(prec, K, trans, g, c->stream);
      break;
    case AIRFE_DEBUG_KERNEL_GEMMR:
      if (a->rowidx || !gemmr_applicable(K, trans, g)) refused = "gemmr";
      else launch_gemmr(prec, trans, g, c->stream);
      break;
    case AIRFE_DEBUG_KERNEL_GEMMR_GATHER:
      if (!gemmr_gather_applicable(K, g)) refused = "gemmr_gather";
      else launch_gemmr_gather(prec, g, c->stream);
      break;
    default:
      if (!gemmr_gather128_applicable(g)) refused = "gemmr_gather128";
      else launch_gemmr_gather128(prec, g, c->stream);
      break;
  }
  if (refused) rc = fail(c, std::string("debug_linear: ") + refused + " does not apply to this form");
  if (!rc && (hipStreamSynchronize(c->stream) != hipSuccess || launch_status(c))) rc = fail(c, "debug_linear: kernel failed");
  if (!rc) {
    if (epi == EPI_STORE_F32 || d2s) {
      std::vector<float> ho(d2s ? (size_t)M * 64 : (size_t)Mp * ldo);
      (void)hipMemcpy(ho.data(), g.out, ho.size() * 4, hipMemcpyDeviceToHost);
      if (d2s) memcpy(a->out, ho.data(), ho.size() * 4);
      else
        for (int m = 0; m < M; ++m) memcpy(a->out + (size_t)m * N, ho.data() + (size_t)m * ldo, (size_t)N * 4);
      if (d2s && a->flag) (void)hipMemcpy(a->flag, g.flag, sizeof(int), hipMemcpyDeviceToHost);
    } else if (heads) {
      std::vector<uint16_t> ho(out_elems);
      const size_t n = (size_t)S * 4 * a->Np * 64;
      (void)hipMemcpy(ho.data(), g.out, ho.size() * 2, hipMemcpyDeviceToHost);
      dbg_back2(ho, n, prec, a->out);
      if (g.out2) {
        (void)hipMemcpy(ho.data(), g.out2, ho.size() * 2, hipMemcpyDeviceToHost);
        dbg_back2(ho, n, prec, a->out2);
      }
    } else {
      std::vector<uint16_t> ho(out_elems);
      (void)hipMemcpy(ho.data(), g.out, ho.size() * 2, hipMemcpyDeviceToHost);
      for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) a->out[(size_t)m * N + n] = back2(ho[(size_t)m * ldo + n], prec);
      if (epi == EPI_RESID) (void)hipMemcpy(a->x32, g.x32, (size_t)M * N * 4, hipMemcpyDeviceToHost);
    }
  }
  return rc;
} AIRFE_CATCH(c)

int airfe_debug_qkv(airfe_ctx* c, int prec, int M, int Np, const float* x, const float* wqk, const float* bqk, int nqk, const float* wv, const float* bv,
                    const float* rot_cos, const float* rot_sin, int pair, int gr_wgs, float* q, float* k, float* vt) try {
  AIRFE_ENTER(c);
  if ((prec != 0 && prec != 1) || M < 1 || Np < 16 || Np % 16 || M % Np || (nqk != 256 && nqk != 512) || !x || !wqk || !bqk || !wv || !bv || !q || !vt ||
      (nqk == 512 && !k) || (!rot_cos) != (!rot_sin))
    return fail(c, "debug_qkv: bad argument");
  const int Mp = (M + 127) / 128 * 128, Sg = (Mp + Np - 1) / Np, S = M / Np;
  const size_t elems = (size_t)Sg * 4 * Np * 64, n = (size_t)S * 4 * Np * 64;
  DbgTmp t(prec);
  airfe_ctx& tmp = t.h;
  LinW lqk, lv;
  const bool packed = make_linear(&tmp, wqk, bqk, 256, nqk, lqk) && make_linear(&tmp, wv, bv, 256, 256, lv);
  GemmArgs ga, gb;
  const uint16_t* dx = dupload(&tmp, dbg_rows2(x, M, 256, Mp, prec));
  ga.X1 = gb.X1 = dx; ga.ld1 = gb.ld1 = 256; ga.K1 = gb.K1 = 256; ga.M = gb.M = Mp; ga.Np = gb.Np = Np; ga.H = gb.H = 4;
  ga.Wp = lqk.w; ga.bias = lqk.b; ga.N = nqk; ga.cb_total = lqk.cbt; ga.epi = EPI_HEADS; ga.ldo = nqk;
  gb.Wp = lv.w; gb.bias = lv.b; gb.N = 256; gb.cb_total = lv.cbt; gb.epi = EPI_HEADS_T; gb.ldo = 256;
  ga.out = dbg_canary<uint16_t>(&tmp, elems);
  if (nqk == 512) ga.out2 = dbg_canary<uint16_t>(&tmp, elems);
  gb.out = dbg_canary<uint16_t>(&tmp, elems);
  if (rot_cos) { ga.rot_cos = dupload(&tmp, dbg_rows4(rot_cos, M, 32, Mp)); ga.rot_sin = dupload(&tmp, dbg_rows4(rot_sin, M, 32, Mp)); }
  for (GemmArgs* g : {&ga, &gb}) {
    g->small_max = c->gemm_small_max; g->g8_min = c->gemm8_min; g->gr_min = c->gemmr_min; g->gr_wgs = gr_wgs > 0 ? gr_wgs : c->gemmr_wgs;
  }
  int rc = (packed && dx && ga.out && gb.out && (nqk != 512 || ga.out2) && (!rot_cos || (ga.rot_cos && ga.rot_sin))) ? 0 : fail(c, "debug_qkv: allocation failed");
  if (!rc) {
    if (pair) {
      if (!gemmr_pair_applicable(ga, gb)) rc = fail(c, "debug_qkv: gemmr_pair does not apply to this form");
      else launch_gemmr_pair(prec, ga, gb, c->stream);
    } else {
      launch_gemm(prec, 256, false, ga, c->stream);
      launch_gemm(prec, 256, true, gb, c->stream);
    }
  }
  if (!rc && (hipStreamSynchronize(c->stream) != hipSuccess || launch_status(c))) rc = fail(c, "debug_qkv: kernel failed");
  if (!rc) {
    std::vector<uint16_t> ho(elems);
    (void)hipMemcpy(ho.data(), ga.out, elems * 2, hipMemcpyDeviceToHost);
    dbg_back2(ho, n, prec, q);
    if (nqk == 512) {
      (void)hipMemcpy(ho.data(), ga.out2, elems * 2, hipMemcpyDeviceToHost);
      dbg_back2(ho, n, prec, k);
    }
    (void)hipMemcpy(ho.data(), gb.out, elems * 2, hipMemcpyDeviceToHost);
    dbg_back2(ho, n, prec, vt);
  }
  return rc;
} AIRFE_CATCH(c)

int airfe_debug_lg_block(airfe_ctx* c, airfe_debug_lg_block_args* a) try {
  AIRFE_ENTER(c);
  if (!a || !a->attn || !a->x32 || !a->xb || !a->w1 || !a->b1 || !a->w2 || !a->b2 || (!a->relu && (!a->gamma || !a->beta)) || (!a->wo) != (!a->bo))
    return fail(c, "debug_lg_block: null argument");
  const int prec = a->prec, M = a->M, T = a->tokens_per_wg, nq = a->nqk_n, Np = a->Np;
  if ((prec != 0 && prec != 1) || M < 1 || (T != 32 && T != 64 && T != 112 && T != 128) || (nq != 0 && nq != 256 && nq != 512) || (a->relu && nq))
    return fail(c, "debug_lg_block: bad argument");
  if (a->mixed) {                                        // the two-round split or nothing: launch_lg_blockf would quietly run uniform passes
    const int tiles = (M + 15) / 16, W = c->n_cu;
    if (a->wo || T != 112 || W <= 0 || tiles <= 7 * W || tiles > 13 * W) return fail(c, "debug_lg_block: the mixed split does not apply to this form");
  }
  if (nq && (!a->nqk_w || !a->nqk_b || !a->nv_w || !a->nv_b || !a->q || !a->vt || (nq == 512) != (a->rot_cos && a->rot_sin) || (nq == 512 && !a->k) || Np < 16 ||
             Np % 16 || M % Np))
    return fail(c, "debug_lg_block: the next projection needs its weights and outputs, rotary exactly when nqk_n = 512, and M = S * Np (Np a multiple of 16)");
  const int cap = M + 256;                               // every pass form stays below M + 127 rows
  const int Sg = nq ? (cap + Np - 1) / Np : 0, S = nq ? M / Np : 0;
  const size_t helems = (size_t)Sg * 4 * Np * 64;
  DbgTmp t(prec);
  airfe_ctx& tmp = t.h;
  LinW lo, l1, l2, lq, lv;
  bool ok = (!a->wo || make_linear(&tmp, a->wo, a->bo, 256, 256, lo)) && make_linear(&tmp, a->w1, a->b1, 512, 512, l1) && make_linear(&tmp, a->w2, a->b2, 512, 256, l2) &&
            (!nq || (make_linear(&tmp, a->nqk_w, a->nqk_b, 256, nq, lq) && make_linear(&tmp, a->nv_w, a->nv_b, 256, 256, lv)));
  const bool fr = lg_blockf_frag_weights();
  std::vector<float> x32h = dbg_rows4(a->x32, M, 256, cap);
  std::vector<uint16_t> xbh((size_t)cap * 256);
  for (size_t i = 0; i < xbh.size(); ++i) xbh[i] = cvt2(x32h[i], prec);
  std::vector<float> gb(1024, 0.f);
  if (!a->relu) { memcpy(gb.data(), a->gamma, 512 * 4); memcpy(gb.data() + 512, a->beta, 512 * 4); }
  LgBlockFArgs g;
  g.attn = dupload(&tmp, dbg_rows2(a->attn, M, 256, cap, prec));
  g.xb = dupload(&tmp, xbh);
  g.x32 = dupload(&tmp, x32h);
  const float* dgb = dupload(&tmp, gb);
  g.wo = a->wo ? (fr ? lo.wf : lo.w) : nullptr; g.bo = a->wo ? lo.b : nullptr;
  g.w1 = fr ? l1.wf : l1.w; g.b1 = l1.b; g.w2 = fr ? l2.wf : l2.w; g.b2 = l2.b;
  g.gamma = dgb; g.beta = dgb ? dgb + 512 : nullptr;
  g.M = M; g.tokens_per_wg = T; g.mixed = a->mixed; g.n_cu = c->n_cu; g.relu = a->relu;
  if (nq) {
    g.nqk_w = fr ? lq.wf : lq.w; g.nqk_b = lq.b; g.nqk_n = nq; g.nv_w = fr ? lv.wf : lv.w; g.nv_b = lv.b; g.Np = Np; g.H = 4;
    if (nq == 512) { g.rot_cos = dupload(&tmp, dbg_rows4(a->rot_cos, M, 32, cap)); g.rot_sin = dupload(&tmp, dbg_rows4(a->rot_sin, M, 32, cap)); }
    g.q_out = dbg_canary<uint16_t>(&tmp, helems);
    if (nq == 512) g.k_out = dbg_canary<uint16_t>(&tmp, helems);
    g.vt_out = dbg_canary<uint16_t>(&tmp, helems);
  }
  ok = ok && g.attn && g.xb && g.x32 && dgb && (!nq || (g.q_out && g.vt_out && (nq != 512 || (g.k_out && g.rot_cos && g.rot_sin))));
  int rc = ok ? 0 : fail(c, "debug_lg_block: allocation failed");
  if (!rc) {
    launch_lg_blockf(prec, g, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess || launch_status(c)) rc = fail(c, "debug_lg_block: kernel failed");
  }
  if (!rc) {
    // rows past M that the launch changed: x32 / xb against their initial (zero) rows, q / k / v^T against the 0xFFFF fill
    std::vector<float> x32o((size_t)cap * 256);
    std::vector<uint16_t> xbo((size_t)cap * 256);
    (void)hipMemcpy(x32o.data(), g.x32, x32o.size() * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(xbo.data(), g.xb, xbo.size() * 2, hipMemcpyDeviceToHost);
    memcpy(a->x32, x32o.data(), (size_t)M * 256 * 4);
    dbg_back2(xbo, (size_t)M * 256, prec, a->xb);
    for (int i = 0; i < 5; ++i) a->rows_past[i] = 0;
    for (int r = M; r < cap; ++r)
      for (int f = 0; f < 256; ++f) {
        const size_t e = (size_t)r * 256 + f;
        if (memcmp(&x32o[e], &x32h[e], 4)) a->rows_past[0] = r - M + 1;
        if (xbo[e] != xbh[e]) a->rows_past[1] = r - M + 1;
      }
    if (nq) {
      uint16_t* dev[3] = {g.q_out, g.k_out, g.vt_out};
      float* host[3] = {a->q, a->k, a->vt};
      std::vector<uint16_t> ho(helems);
      for (int j = 0; j < 3; ++j) {
        if (!dev[j]) continue;
        (void)hipMemcpy(ho.data(), dev[j], helems * 2, hipMemcpyDeviceToHost);
        dbg_back2(ho, (size_t)S * 4 * Np * 64, prec, host[j]);
        for (size_t e = (size_t)S * 4 * Np * 64; e < helems; ++e) {
          if (ho[e] == 0xFFFF) continue;
          const size_t s = e / ((size_t)4 * Np * 64), w = e % ((size_t)Np * 64);
          const int row = (int)(s * Np + (j == 2 ? w % Np : w / 64));          // q / k [s][h][n][64], v^T [s][h][d][n]
          a->rows_past[2 + j] = std::max(a->rows_past[2 + j], row - M + 1);
        }
      }
    }
  }
  return rc;
} AIRFE_CATCH(c)

int airfe_debug_ln_gelu(airfe_ctx* c, int prec, float* h, const float* gamma, const float* beta, int M) try {
  AIRFE_ENTER(c);
  if ((prec != 0 && prec != 1) || M < 1 || !h || !gamma || !beta) return fail(c, "debug_ln_gelu: bad argument");
  DbgTmp t;
  airfe_ctx& tmp = t.h;
  std::vector<float> gb(1024);
  memcpy(gb.data(), gamma, 512 * 4);
  memcpy(gb.data() + 512, beta, 512 * 4);
  uint16_t* dh = dupload(&tmp, dbg_rows2(h, M, 512, M, prec));
  float* dgb = dupload(&tmp, gb);
  int rc = dh && dgb ? 0 : fail(c, "debug_ln_gelu: allocation failed");
  if (!rc) {
    launch_ln_gelu(prec, dh, dgb, dgb + 512, M, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess || launch_status(c)) rc = fail(c, "debug_ln_gelu: kernel failed");
  }
  if (!rc) {
    std::vector<uint16_t> ho((size_t)M * 512);
    (void)hipMemcpy(ho.data(), dh, ho.size() * 2, hipMemcpyDeviceToHost);
    dbg_back2(ho, ho.size(), prec, h);
  }
  return rc;
} AIRFE_CATCH(c)
}  // extern "C"

// the body of both attention hooks (the callers hold the context and catch)
static int dbg_attention_run(airfe_ctx* c, airfe_debug_attn_args* a, const char* who) {
  const std::string w = std::string(who) + ": ";
  const int S = a->S, H = a->H, n = a->n, cross = a->cross, prec = a->prec;
  if (prec != 0 && prec != 1) return fail(c, w + "prec must be 0 (bf16) or 1 (fp16)");
  if (S < 1 || H < 1 || n < 1 || (S * H) % 8 != 0 || (cross && (S & 1))) return fail(c, w + "S * H must be a multiple of 8 (cross: S even)");
  if (!a->q || !a->k || !a->v || !a->lens || !a->out) return fail(c, w + "null argument");
  for (int s = 0; s < S; ++s)
    if (a->lens[s] < 0 || a->lens[s] > n) return fail(c, w + "lens[s] must lie in 0 .. n");
  const int Np = (n + 15) / 16 * 16;
  a->Np = Np; a->rows_past = 0;
  const size_t rows = (size_t)S * H * Np + 128;                      // (+ slack: the last key tile reads up to 63 rows past a sequence; it stays ZERO like the arena's)
  std::vector<uint16_t> hq(rows * 64, 0), hk(rows * 64, 0), hvt(rows * 64, 0);
  for (int s = 0; s < S; ++s)
    for (int h = 0; h < H; ++h)
      for (int i = 0; i < n; ++i)
        for (int d = 0; d < 64; ++d) {
          const size_t src = (((size_t)s * H + h) * n + i) * 64 + d;
          hq[(((size_t)s * H + h) * Np + i) * 64 + d] = cvt2(a->q[src], prec);
          hk[(((size_t)s * H + h) * Np + i) * 64 + d] = cvt2(a->k[src], prec);
          hvt[(((size_t)s * H + h) * 64 + d) * Np + i] = cvt2(a->v[src], prec);       // V^T [S][H][64][Np]
        }
  DbgTmp t;
  airfe_ctx* tmp = &t.h;   // only as an allocation list holder
  uint16_t *dq = dupload(tmp, hq), *dk = dupload(tmp, hk), *dv = dupload(tmp, hvt);
  const size_t out_n = (size_t)S * Np * H * 64, slack_n = (size_t)128 * H * 64;
  uint16_t* dout = dalloc<uint16_t>(tmp, out_n + slack_n);
  std::vector<int> hl(a->lens, a->lens + S);
  int* dl = dupload(tmp, hl);
  if (!dq || !dk || !dv || !dout || !dl) return fail(c, w + "allocation failed");
  if (a->canary && hipMemsetAsync(dout, 0xFF, (out_n + slack_n) * 2, c->stream) != hipSuccess) return fail(c, w + "memset failed");
  launch_attention32(prec, dq, dk, dv, dout, dl, S, H, Np, cross, c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess || launch_status(c)) return fail(c, w + "kernel failed");
  std::vector<uint16_t> ho(out_n + slack_n);
  if (hipMemcpy(ho.data(), dout, ho.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, w + "copy failed");
  const int rows_out = a->raw ? Np : n;
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < rows_out; ++i)
      for (int f = 0; f < H * 64; ++f) a->out[((size_t)s * rows_out + i) * H * 64 + f] = back2(ho[((size_t)s * Np + i) * H * 64 + f], prec);
  if (a->canary)
    for (int r = 0; r < 128; ++r) {
      bool changed = false;
      for (int f = 0; f < H * 64 && !changed; ++f) changed = ho[out_n + (size_t)r * H * 64 + f] != 0xFFFFu;
      a->rows_past += changed;
    }
  return 0;
}

extern "C" {
int airfe_debug_attention(airfe_ctx* c, const float* q, const float* k, const float* v, const int* lens, int S, int H, int n, int cross, float* out) try {
  AIRFE_ENTER(c);
  if (c->mprec == 2) return fail(c, "debug_attention drives the 2-byte kernel (matcher_precision fp16 / bf16)");
  airfe_debug_attn_args a = {};
  a.prec = c->mprec; a.S = S; a.H = H; a.n = n; a.cross = cross;
  a.q = q; a.k = k; a.v = v; a.lens = lens; a.out = out;                 // canary = 0, raw = 0: the output buffer as the allocator left it, the first n rows back
  return dbg_attention_run(c, &a, "debug_attention");
} AIRFE_CATCH(c)

int airfe_debug_attention_args(airfe_ctx* c, airfe_debug_attn_args* a) try {
  AIRFE_ENTER(c);
  if (!a) return fail(c, "debug_attention_args: null argument");
  return dbg_attention_run(c, a, "debug_attention_args");
} AIRFE_CATCH(c)

/* ---- LightGlue's head and tail one launcher at a time (include/airfe_debug.h; tests/test_gpu_lg_tail.py) */
int airfe_debug_lg_prepare(airfe_ctx* c, airfe_debug_lg_prepare_args* a) try {
  AIRFE_ENTER(c);
  if (!c->has_arena) return fail(c, "debug_lg_prepare: no matcher loaded");
  if (!a || !a->f0 || !a->f1 || !a->n0 || !a->n1 || !a->wr || !a->x32 || !a->xb || !a->rot_cos || !a->rot_sin || !a->lens || (!a->f0x) != (!a->f1x))
    return fail(c, "debug_lg_prepare: null argument");
  const int Np = c->Np, B = a->B, Bt = a->f0x ? 2 : B;
  if ((a->prec != 0 && a->prec != 1) || B < 1 || B > c->Pmax || (a->f0x && (B != 1 || c->Pmax < 2)) || a->cap < 1 || a->cap > Np || a->kp_off < 0 ||
      a->ld < a->kp_off + 258 || a->slack_rows < 0)
    return fail(c, "debug_lg_prepare: bad argument (prec 0 / 1, 1 <= B <= max_batch, a second pair with B = 1 only, 1 <= cap <= Np, ld >= kp_off + 258)");
  for (int b = 0; b < B; ++b)
    if (a->n0[b] < 0 || a->n0[b] > a->cap || a->n1[b] < 0 || a->n1[b] > a->cap) return fail(c, "debug_lg_prepare: every n0, n1 must lie in 0 .. cap");
  if (a->f0x && (a->n0x < 0 || a->n0x > Np || a->n1x < 0 || a->n1x > Np)) return fail(c, "debug_lg_prepare: the second pair's lengths must lie in 0 .. Np");
  const size_t rows = (size_t)2 * Bt * Np + (size_t)a->slack_rows, R = c->arena_rows;
  if (rows > R || (size_t)a->rows != rows) return fail(c, "debug_lg_prepare: rows must be 2 Bt Np + slack_rows and fit the arena");
  DbgTmp t;
  const size_t fl = (size_t)B * a->cap * a->ld;
  std::vector<float> hf0(a->f0, a->f0 + fl), hf1(a->f1, a->f1 + fl), hwr(a->wr, a->wr + 64);
  std::vector<int> hn(2 * B + 2);
  for (int b = 0; b < B; ++b) { hn[b] = a->n0[b]; hn[B + b] = a->n1[b]; }
  hn[2 * B] = a->n0x; hn[2 * B + 1] = a->n1x;
  float *df0 = dupload(&t.h, hf0), *df1 = dupload(&t.h, hf1), *dwr = dupload(&t.h, hwr), *df0x = nullptr, *df1x = nullptr;
  int* dn = dupload(&t.h, hn);
  if (a->f0x) {
    std::vector<float> x0(a->f0x, a->f0x + (size_t)a->n0x * a->ld), x1(a->f1x, a->f1x + (size_t)a->n1x * a->ld);
    x0.resize(x0.size() + a->ld, 0.f); x1.resize(x1.size() + a->ld, 0.f);          // (never empty)
    df0x = dupload(&t.h, x0); df1x = dupload(&t.h, x1);
    if (!df0x || !df1x) return fail(c, "debug_lg_prepare: allocation failed");
  }
  if (!df0 || !df1 || !dwr || !dn) return fail(c, "debug_lg_prepare: allocation failed");
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemsetAsync(c->x32, 0xFF, R * 256 * 4, st));
  HIPCHK(c, hipMemsetAsync(c->xb, 0xFF, R * 256 * 2, st));
  HIPCHK(c, hipMemsetAsync(c->rot_cos, 0xFF, R * 32 * 4, st));
  HIPCHK(c, hipMemsetAsync(c->rot_sin, 0xFF, R * 32 * 4, st));
  HIPCHK(c, hipMemsetAsync(c->lens, 0xFF, (size_t)2 * c->Pmax * 4, st));
  LgPrepArgs pa;
  pa.f0 = df0; pa.f1 = df1; pa.n0 = dn; pa.n1 = dn + B; pa.ld = a->ld; pa.kp_off = a->kp_off; pa.normalize = a->normalize;
  pa.cx = a->cx; pa.cy = a->cy; pa.linv = a->linv; pa.wr = dwr; pa.B = B; pa.cap = a->cap; pa.Np = Np;
  pa.x32 = c->x32; pa.xb = c->xb; pa.rot_cos = c->rot_cos; pa.rot_sin = c->rot_sin; pa.lens = c->lens;
  if (a->f0x) { pa.f0x = df0x; pa.f1x = df1x; pa.n0x = dn + 2 * B; pa.n1x = dn + 2 * B + 1; }
  pa.slack_rows = a->slack_rows;
  launch_lg_prepare(a->prec, pa, st);
  HIPCHK(c, hipStreamSynchronize(st));
  if (launch_status(c)) return 1;
  std::vector<float> hx(R * 256);
  std::vector<uint16_t> hb(R * 256);
  HIPCHK(c, hipMemcpy(hx.data(), c->x32, hx.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(hb.data(), c->xb, hb.size() * 2, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->rot_cos, c->rot_cos, rows * 32 * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->rot_sin, c->rot_sin, rows * 32 * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->lens, c->lens, (size_t)2 * Bt * 4, hipMemcpyDeviceToHost));
  memcpy(a->x32, hx.data(), rows * 256 * 4);
  dbg_back2(hb, rows * 256, a->prec, a->xb);
  int past = 0;
  for (size_t r = rows; r < R; ++r) {
    bool touched = false;
    for (int k = 0; k < 256 && !touched; ++k) {
      uint32_t u;
      memcpy(&u, &hx[r * 256 + k], 4);
      touched = u != 0xFFFFFFFFu || hb[r * 256 + k] != 0xFFFFu;
    }
    past += touched;
  }
  a->rows_past = past;
  // the arena as alloc_matcher_arena left it: the pipelines reset only the slack rows their own kernels can reach
  HIPCHK(c, hipMemsetAsync(c->x32, 0, R * 256 * 4, st));
  HIPCHK(c, hipMemsetAsync(c->xb, 0, R * 256 * 2, st));
  HIPCHK(c, hipMemsetAsync(c->rot_cos, 0, R * 32 * 4, st));
  HIPCHK(c, hipMemsetAsync(c->rot_sin, 0, R * 32 * 4, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_lg_assign(airfe_ctx* c, airfe_debug_lg_assign_args* a) try {
  AIRFE_ENTER(c);
  if (!c->has_arena) return fail(c, "debug_lg_assign: no matcher loaded");
  if (!a || !a->md || !a->x32 || !a->w || !a->lens || !a->z || !a->sim || !a->scores || !a->rowlse || !a->collse || !a->rowval || !a->rowarg || !a->colarg ||
      !a->idx || !a->score || !a->nmatch)
    return fail(c, "debug_lg_assign: null argument");
  const int Np = c->Np, B = a->B, n = a->n, S = 2 * B, cap = a->cap, prec = a->prec;
  if ((prec != 0 && prec != 1) || B < 1 || B > c->Pmax || n < 1 || n > Np || cap < 1 || cap > Np || (a->form != 0 && a->form != 1))
    return fail(c, "debug_lg_assign: bad argument (prec 0 / 1, 1 <= B <= max_batch, 1 <= n, cap <= Np, form 0 / 1)");
  for (int s = 0; s < S; ++s)
    if (a->lens[s] < 0 || a->lens[s] > n) return fail(c, "debug_lg_assign: every length must lie in 0 .. n");
  const size_t M = (size_t)S * Np, blk = (size_t)Np * Np, pf = lg_assign_part_floats(B, Np);
  std::vector<uint16_t> hmd(M * 256, 0xFFFFu);
  std::vector<float> hx(M * 256);
  memset(hx.data(), 0xFF, hx.size() * 4);
  for (int s = 0; s < S; ++s) {
    for (int i = 0; i < a->lens[s]; ++i)
      for (int k = 0; k < 256; ++k) {
        hmd[((size_t)s * Np + i) * 256 + k] = cvt2(a->md[((size_t)s * n + i) * 256 + k], prec);
        hx[((size_t)s * Np + i) * 256 + k] = a->x32[((size_t)s * n + i) * 256 + k];
      }
    if (a->pad)
      for (int i = a->lens[s]; i < Np; ++i)
        for (int k = 0; k < 256; ++k) hmd[((size_t)s * Np + i) * 256 + k] = cvt2(a->pad[k], prec);
  }
  DbgTmp t;
  std::vector<float> hw(a->w, a->w + 256);
  float* dw = dupload(&t.h, hw);
  float* dscores = dalloc<float>(&t.h, (size_t)B * blk, false);
  int32_t* didx = dalloc<int32_t>(&t.h, (size_t)B * cap * 2, false);
  float* dscore = dalloc<float>(&t.h, (size_t)B * cap, false);
  int* dnm = dalloc<int>(&t.h, (size_t)B, false);
  if (!dw || !dscores || !didx || !dscore || !dnm) return fail(c, "debug_lg_assign: allocation failed");
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->mdb, hmd.data(), hmd.size() * 2, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->x32, hx.data(), hx.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->lens, a->lens, (size_t)S * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(c->zbuf, 0xFF, M * 4, st));
  HIPCHK(c, hipMemsetAsync(c->simbuf, 0xFF, (size_t)B * blk * 4, st));
  HIPCHK(c, hipMemsetAsync(c->lg_part, 0xFF, pf * 4, st));
  HIPCHK(c, hipMemsetAsync(c->lg_argpart, 0xFF, pf * 4, st));
  HIPCHK(c, hipMemsetAsync(c->rowlse, 0xFF, (size_t)B * Np * 4, st));
  HIPCHK(c, hipMemsetAsync(c->collse, 0xFF, (size_t)B * Np * 4, st));
  HIPCHK(c, hipMemsetAsync(c->rowval, 0xFF, (size_t)B * Np * 4, st));
  HIPCHK(c, hipMemsetAsync(dscores, 0xFF, (size_t)B * blk * 4, st));
  HIPCHK(c, hipMemsetAsync(dscore, 0xFF, (size_t)B * cap * 4, st));
  HIPCHK(c, hipMemsetAsync(dnm, 0xFF, (size_t)B * 4, st));
  HIPCHK(c, hipMemsetAsync(c->rowarg, 0, (size_t)B * Np * 4, st));          // zero, not -1: the value that passes for a valid index
  HIPCHK(c, hipMemsetAsync(c->colarg, 0, (size_t)B * Np * 4, st));
  HIPCHK(c, hipMemsetAsync(didx, 0, (size_t)B * cap * 8, st));
  launch_rowdot256(c->x32, dw, a->b, c->zbuf, (int)M, st);
  if (a->form == 1) {
    launch_lg_assign_fused(prec, c->mdb, c->zbuf, c->lens, B, Np, cap, a->thr, c->lg_part, c->lg_argpart, c->rowlse, c->collse, c->simbuf, dscores, c->rowarg,
                           c->rowval, c->colarg, didx, dscore, dnm, st);
  } else {
    launch_sim(prec, c->mdb, c->simbuf, B, Np, st);
    launch_lg_assign(c->simbuf, c->zbuf, c->lens, B, Np, cap, a->thr, c->rowlse, c->collse, dscores, c->rowarg, c->rowval, c->colarg, didx, dscore, dnm, st);
  }
  HIPCHK(c, hipStreamSynchronize(st));
  if (launch_status(c)) return 1;
  const size_t nb = (size_t)n * 4, npb = (size_t)Np * 4;
  HIPCHK(c, hipMemcpy2D(a->z, nb, c->zbuf, npb, nb, S, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    HIPCHK(c, hipMemcpy2D(a->sim + (size_t)b * n * n, nb, c->simbuf + b * blk, npb, nb, n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy2D(a->scores + (size_t)b * n * n, nb, dscores + b * blk, npb, nb, n, hipMemcpyDeviceToHost));
  }
  HIPCHK(c, hipMemcpy2D(a->rowlse, nb, c->rowlse, npb, nb, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy2D(a->collse, nb, c->collse, npb, nb, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy2D(a->rowval, nb, c->rowval, npb, nb, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy2D(a->rowarg, nb, c->rowarg, npb, nb, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy2D(a->colarg, nb, c->colarg, npb, nb, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->idx, didx, (size_t)B * cap * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->score, dscore, (size_t)B * cap * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->nmatch, dnm, (size_t)B * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemsetAsync(c->mdb, 0, M * 256 * 2, st));          // no NaN token rows stay behind
  HIPCHK(c, hipMemsetAsync(c->x32, 0, M * 256 * 4, st));
  HIPCHK(c, hipMemsetAsync(c->zbuf, 0, M * 4, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
} AIRFE_CATCH(c)

/* ---- the detector's and the line path's index work on hand-built maps (include/airfe_debug.h; tests/test_gpu_detector_tail_pin.py, tests/detector_tail_ref.py).  HOST tensors
 * staged into the context's own buffers, then the steps production is composed of (airfe_detect.hip, airfe_lines.hip: each launch sequence is stated there once, the hooks call it;
 * tests/test_line_path_one_statement_cpu.py); nothing here has a kernel or a line-path launch of its own. */
int airfe_debug_detector_tail(airfe_ctx* c, airfe_debug_detector_tail_args* a) try {
  AIRFE_ENTER(c);
  if (!c->has_sp) return fail(c, "debug_detector_tail: detector not loaded");
  if (c->prec != 0 && c->prec != 1) return fail(c, "debug_detector_tail drives the 2-byte detector (cfg.precision fp16 / bf16)");
  if (!a || !a->heat || !a->act || !a->feat || !a->n) return fail(c, "debug_detector_tail: null argument");
  const int B = a->B, Bs = a->Bs, cap = a->cap, R = AIRFE_INTERNAL_SIZE;
  const bool two = Bs != 0;
  if (B < 1 || B > c->Dmax || (two && (B != 2 * Bs || Bs > c->Bmax || !a->feat1 || !a->n1)) || (!two && B > c->Bmax))
    return fail(c, "debug_detector_tail: 1 <= B <= max_batch, or B = 2 Bs with both destinations given");
  if (a->h < 1 || a->w < 1 || cap < c->cfg.max_keypoints) return fail(c, "debug_detector_tail: empty image or feature capacity < max_keypoints");
  if (a->keep && c->cfg.nms_radius != 4) return fail(c, "debug_detector_tail: the keep plane exists on the radius-4 path only");
  const size_t px = (size_t)B * R * R, cells = (size_t)B * (R / 8) * (R / 8);
  for (size_t i = 0; i < px; ++i)
    if (!(a->heat[i] >= 0.f && a->heat[i] <= 1.f)) return fail(c, "debug_detector_tail: scores must lie in [0, 1]");
  std::vector<uint16_t> act(cells * 256);
  for (size_t i = 0; i < act.size(); ++i) act[i] = cvt2(a->act[i], c->prec);
  const int B0 = two ? Bs : B, B1 = two ? B - Bs : 0;
  DbgTmp t;
  float* dfeat = dupload(&t.h, std::vector<float>(a->feat, a->feat + (size_t)B0 * cap * AIRFE_FEAT_DIM));
  int* dn = dupload(&t.h, std::vector<int>(a->n, a->n + B0));
  float* dfeat1 = two ? dupload(&t.h, std::vector<float>(a->feat1, a->feat1 + (size_t)B1 * cap * AIRFE_FEAT_DIM)) : nullptr;
  int* dn1 = two ? dupload(&t.h, std::vector<int>(a->n1, a->n1 + B1)) : nullptr;
  if (!dfeat || !dn || (two && (!dfeat1 || !dn1))) return fail(c, "debug_detector_tail: allocation failed");
  hipStream_t st = c->stream;
  clear_saturation(c);
  HIPCHK(c, hipMemcpyAsync(c->heat, a->heat, px * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->aDa, act.data(), act.size() * 2, hipMemcpyHostToDevice, st));
  // detect_dev2's descriptor-head rule (point_desc_head), then its tail
  bool sparse_desc = false;
  if (point_desc_head(c, B, cap, st, sparse_desc)) { (void)hipStreamSynchronize(st); return 1; }
  const int rc = detect_tail_dev(c, B, Bs, two, sparse_desc, a->h, a->w, dfeat, dfeat1, cap, dn, dn1, st);
  HIPCHK(c, hipStreamSynchronize(st));                       // (act goes out of scope)
  if (rc) return 1;
  if (saturation_status(c)) return 1;
  HIPCHK(c, hipMemcpy(a->feat, dfeat, (size_t)B0 * cap * AIRFE_FEAT_DIM * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->n, dn, (size_t)B0 * 4, hipMemcpyDeviceToHost));
  if (two) {
    HIPCHK(c, hipMemcpy(a->feat1, dfeat1, (size_t)B1 * cap * AIRFE_FEAT_DIM * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(a->n1, dn1, (size_t)B1 * 4, hipMemcpyDeviceToHost));
  }
  a->nms_map_written = c->cfg.nms_radius > 0 && c->nms_map_valid;
  if (a->nms_map && a->nms_map_written) HIPCHK(c, hipMemcpy(a->nms_map, c->heat_nms, px * 4, hipMemcpyDeviceToHost));
  if (a->keep) HIPCHK(c, hipMemcpy(a->keep, c->nms_mask, cells * 8, hipMemcpyDeviceToHost));
  if (a->cand_cnt) HIPCHK(c, hipMemcpy(a->cand_cnt, c->cand_cnt, (size_t)B * 4, hipMemcpyDeviceToHost));
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_line_post(airfe_ctx* c, airfe_debug_line_post_args* a) try {
  AIRFE_ENTER(c);
  if (!c->has_sp || !c->has_s1 || !c->s1_la || !c->jmap) return fail(c, "debug_line_post: the line path is not loaded (cfg.plnet_s1_pack)");
  if (c->cfg.nms_radius != 4) return fail(c, "debug_line_post: both junction score sources exist on the radius-4 path only");
  if (!a || !a->la || !a->sc || !a->m2 || !a->heat || !a->lines || !a->nlines || !a->nfound) return fail(c, "debug_line_post: null argument");
  const int B = a->B, nj = a->nj, ld = a->ld, capL = a->capL, capJ = a->capJ, R = AIRFE_INTERNAL_SIZE;
  if (B < 1 || B > c->Lmax || B > c->Dmax || nj < 0 || nj > B || ld < 1 || ld > LINE_CAP || capL < 1 || capJ < 1 || a->h < 1 || a->w < 1)
    return fail(c, "debug_line_post: bad argument (1 <= B <= the arena's images, 0 <= nj <= B, 1 <= ld <= 45056, capL, capJ >= 1)");
  if (nj > 0 && (!a->junc || !a->njunc || !a->jfound)) return fail(c, "debug_line_post: nj > 0 needs the junction outputs");
  for (int b = 0; b < B; ++b)
    if (a->m2[b] < 0 || a->m2[b] > ld) return fail(c, "debug_line_post: every m2 must lie in 0 .. ld");
  DbgTmp t;
  double* dlines = dupload(&t.h, std::vector<double>(a->lines, a->lines + (size_t)B * capL * 4));
  float* djunc = nj > 0 ? dupload(&t.h, std::vector<float>(a->junc, a->junc + (size_t)nj * capJ * AIRFE_FEAT_DIM)) : nullptr;
  int* dcnt = dbg_canary<int>(&t.h, (size_t)4 * B);          // nlines | nfound | njunc | jfound
  if (!dlines || (nj > 0 && !djunc) || !dcnt) return fail(c, "debug_line_post: allocation failed");
  hipStream_t st = c->stream;
  clear_saturation(c);
  std::vector<int> counts((size_t)B * LINE_CNT_LD, 0);
  for (int b = 0; b < B; ++b) {
    counts[(size_t)b * LINE_CNT_LD + 1] = a->m2[b];
    HIPCHK(c, hipMemcpyAsync(c->s1_la + (size_t)b * LINE_CAP * 4, a->la + (size_t)b * ld * 4, (size_t)ld * 16, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->s1_sc + (size_t)b * LINE_CAP, a->sc + (size_t)b * ld, (size_t)ld * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, hipMemcpyAsync(c->wf_counts, counts.data(), counts.size() * 4, hipMemcpyHostToDevice, st));
  c->wf_counted = false;                                     // (the per-workgroup counts of a previous line branch are gone)
  HIPCHK(c, hipMemcpyAsync(c->heat, a->heat, (size_t)B * R * R * 4, hipMemcpyHostToDevice, st));
  // the point branch's NMS as detect_tail_dev runs it: with the dense map (one- and two-image calls) or with the keep plane alone (larger batches)
  c->nms_map_valid = !a->from_plane;
  launch_nms512_candidates(c->heat, c->nms_map_valid ? c->heat_nms : nullptr, c->nms_mask, B, c->cfg.keypoint_threshold, c->cfg.remove_borders, c->cand, c->cand_cnt,
                           R * R, st);
  // line_post_dev's steps without the descriptor sampling (line_filter_maps, junction_scan_maps), images 0 .. B-1, junctions of the first nj
  junction_maps_clear(c, nj, st);
  line_filter_maps(c, B, nj, a->h, a->w, dlines, capL, dcnt, dcnt + B, st);
  // a caller's junction maps instead of the filter's, between the two launches: the scan's own bounds (the filter never marks a pixel the scan would reject)
  if (nj > 0 && a->jmap) HIPCHK(c, hipMemcpyAsync(c->jmap, a->jmap, (size_t)nj * R * R, hipMemcpyHostToDevice, st));
  const int rc = nj > 0 ? junction_scan_maps(c, 0, nj, djunc, capJ, dcnt + 2 * B, dcnt + 3 * B, st) : 0;
  HIPCHK(c, hipStreamSynchronize(st));                       // (counts goes out of scope)
  if (rc || launch_status(c)) return 1;
  if (saturation_status(c)) return 1;
  HIPCHK(c, hipMemcpy(a->lines, dlines, (size_t)B * capL * 32, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->nlines, dcnt, (size_t)B * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->nfound, dcnt + B, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (nj > 0) {
    HIPCHK(c, hipMemcpy(a->junc, djunc, (size_t)nj * capJ * AIRFE_FEAT_DIM * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(a->njunc, dcnt + 2 * B, (size_t)nj * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(a->jfound, dcnt + 3 * B, (size_t)nj * 4, hipMemcpyDeviceToHost));
  }
  return 0;
} AIRFE_CATCH(c)

/* the junction tail as the batched entries run it (include/airfe_debug.h): the point branch's state as detect_dev2 leaves it, plnet_lines_batch's rule for the junction
 * images' dense descriptor map (junction_dense_maps), then line_tail_dev's end (line_post_dev, airfe_lines.hip) — in either form, chosen as production chooses it */
int airfe_debug_junction_tail(airfe_ctx* c, airfe_debug_junction_tail_args* a) try {
  AIRFE_ENTER(c);
  if (!c->has_sp || !c->has_s1 || !c->s1_la || !c->jmap) return fail(c, "debug_junction_tail: the line path is not loaded (cfg.plnet_s1_pack)");
  if (c->prec != 0 && c->prec != 1) return fail(c, "debug_junction_tail drives the 2-byte detector (cfg.precision fp16 / bf16)");
  if (c->cfg.nms_radius != 4) return fail(c, "debug_junction_tail: the keep plane exists on the radius-4 path only");
  if (!a || !a->la || !a->sc || !a->m2 || !a->heat || !a->act || !a->lines || !a->nlines || !a->nfound) return fail(c, "debug_junction_tail: null argument");
  const int B = a->B, nj = a->nj, ld = a->ld, capL = a->capL, capJ = a->capJ, R = AIRFE_INTERNAL_SIZE;
  if (B < 1 || B > c->Lmax || B > c->Bmax || nj < 0 || nj > B || ld < 1 || ld > LINE_CAP || capL < 1 || capJ < 1 || a->h < 1 || a->w < 1)
    return fail(c, "debug_junction_tail: bad argument (1 <= B <= max_batch, 0 <= nj <= B, 1 <= ld <= 45056, capL, capJ >= 1)");
  if (nj > 0 && (!a->junc || !a->njunc || !a->jfound)) return fail(c, "debug_junction_tail: nj > 0 needs the junction outputs");
  for (int b = 0; b < B; ++b)
    if (a->m2[b] < 0 || a->m2[b] > ld) return fail(c, "debug_junction_tail: every m2 must lie in 0 .. ld");
  const size_t px = (size_t)B * R * R, cells = (size_t)B * (R / 8) * (R / 8);
  for (size_t i = 0; i < px; ++i)
    if (!(a->heat[i] >= 0.f && a->heat[i] <= 1.f)) return fail(c, "debug_junction_tail: scores must lie in [0, 1]");
  std::vector<uint16_t> act(cells * 256);
  for (size_t i = 0; i < act.size(); ++i) act[i] = cvt2(a->act[i], c->prec);
  DbgTmp t;
  double* dlines = dupload(&t.h, std::vector<double>(a->lines, a->lines + (size_t)B * capL * 4));
  float* djunc = nj > 0 ? dupload(&t.h, std::vector<float>(a->junc, a->junc + (size_t)nj * capJ * AIRFE_FEAT_DIM)) : nullptr;
  int* dcnt = dbg_canary<int>(&t.h, (size_t)4 * B);          // nlines | nfound | njunc | jfound
  if (!dlines || (nj > 0 && !djunc) || !dcnt) return fail(c, "debug_junction_tail: allocation failed");
  hipStream_t st = c->stream;
  clear_saturation(c);
  std::vector<int> counts((size_t)B * LINE_CNT_LD, 0);
  for (int b = 0; b < B; ++b) {
    counts[(size_t)b * LINE_CNT_LD + 1] = a->m2[b];
    HIPCHK(c, hipMemcpyAsync(c->s1_la + (size_t)b * LINE_CAP * 4, a->la + (size_t)b * ld * 4, (size_t)ld * 16, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->s1_sc + (size_t)b * LINE_CAP, a->sc + (size_t)b * ld, (size_t)ld * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, hipMemcpyAsync(c->wf_counts, counts.data(), counts.size() * 4, hipMemcpyHostToDevice, st));
  c->wf_counted = false;
  HIPCHK(c, hipMemcpyAsync(c->heat, a->heat, px * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->aDa, act.data(), act.size() * 2, hipMemcpyHostToDevice, st));
  // the point branch as detect_dev2 / detect_tail_dev leave it: one- and two-image calls keep the dense NMS'd map and the dense descriptor map, larger batches the keep
  // plane alone (their descriptor head ran over the sampled cells)
  c->nms_map_valid = B <= 2;
  launch_nms512_candidates(c->heat, c->nms_map_valid ? c->heat_nms : nullptr, c->nms_mask, B, c->cfg.keypoint_threshold, c->cfg.remove_borders, c->cand, c->cand_cnt,
                           R * R, st);
  c->desc_dense_valid = false;
  c->last_B = B;
  int rc = 0;
  if (B <= 2) {
    rc = dense_desc_head(c, B, st);
    c->desc_dense_valid = true;
  }
  // plnet_lines_batch's rule (junction_dense_maps), then line_tail_dev's clear of the byte maps and its end
  bool partial = false;
  if (!rc) rc = junction_dense_maps(c, nj, capJ, 3, st, partial);
  const bool fused = junction_tail_fused(c, nj, capJ);
  if (!rc && !fused) junction_maps_clear(c, nj, st);
  if (!rc) rc = line_post_dev(c, 0, B, a->h, a->w, dlines, capL, dcnt, dcnt + B, djunc, capJ, dcnt + 2 * B, dcnt + 3 * B, nj, st, 3, fused);
  if (partial) c->desc_dense_valid = false;
  HIPCHK(c, hipStreamSynchronize(st));                       // (counts, act go out of scope)
  if (rc || launch_status(c)) return 1;
  if (saturation_status(c)) return 1;
  a->fused = fused ? 1 : 0;
  HIPCHK(c, hipMemcpy(a->lines, dlines, (size_t)B * capL * 32, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->nlines, dcnt, (size_t)B * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->nfound, dcnt + B, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (nj > 0) {
    HIPCHK(c, hipMemcpy(a->junc, djunc, (size_t)nj * capJ * AIRFE_FEAT_DIM * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(a->njunc, dcnt + 2 * B, (size_t)nj * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(a->jfound, dcnt + 3 * B, (size_t)nj * 4, hipMemcpyDeviceToHost));
  }
  return 0;
} AIRFE_CATCH(c)

/* the line path between the stage-0 tensors and the line filter (include/airfe_debug.h): line_branch_dev's line_match, then line_tail_dev's line_dedup, line_tap_rows and
 * line_stage1 (airfe_lines.hip), on host tensors staged into the stage block and the line-path buffers */
int airfe_debug_line_mid(airfe_ctx* c, airfe_debug_line_mid_args* a) try {
  AIRFE_ENTER(c);
  if (!c->has_sp || !c->has_s0 || !c->has_s1 || !c->s0_stage || !c->l_ta8) return fail(c, "debug_line_mid: the line path is not loaded (line.* tensors, cfg.plnet_s1_pack)");
  if (!a || !a->juncs_pred || !a->lines_pred || !a->thin || !a->aux || !a->loi || !a->iskeep || !a->idx_min || !a->idx_max || !a->counts || !a->keep || !a->pairs || !a->rep ||
      !a->head4 || !a->prop4 || !a->ridx || !a->proj || !a->lines_adjusted || !a->scores_line || !a->table_dirty)
    return fail(c, "debug_line_mid: null argument");
  const int B = a->B, form = a->s1_form, NP = KEEP_CAP, NPX = 128 * 128;
  if (B < 1 || B > c->Lmax) return fail(c, "debug_line_mid: 1 <= B <= the arena's images");
  if (a->j2l < 0 || a->j2l > 2 || form < 0 || form > 3) return fail(c, "debug_line_mid: j2l is 0 .. 2, s1_form 0 .. 3");
  if (form <= 1 && B != 1) return fail(c, "debug_line_mid: forms 0 and 1 (CHW tensors, head rows) hold one image");
  if (a->j2l == 0 && (!a->iskeep_in || !a->idx_min_in || !a->idx_max_in)) return fail(c, "debug_line_mid: j2l = 0 needs iskeep_in, idx_min_in and idx_max_in");
  if (a->wgs < 0 || a->wgs > 512) return fail(c, "debug_line_mid: wgs must lie in 0 .. 512");
  if (form == 3)
    for (int i = 0; i < 6; ++i)
      if (!c->s1_wsplit[i]) return fail(c, "debug_line_mid: form 3 needs the split stage-1 weights");
  for (size_t i = 0; i < (size_t)B * 600; ++i)
    if (!std::isfinite(a->juncs_pred[i])) return fail(c, "debug_line_mid: junction coordinates must be finite");
  for (size_t i = 0; i < (size_t)B * NP * 4; ++i)
    if (!std::isfinite(a->lines_pred[i])) return fail(c, "debug_line_mid: proposal coordinates must be finite");
  hipStream_t st = c->stream;
  float* d = c->s0_stage;
  clear_saturation(c);
  // ---- staging: the stage block (juncs | lines_pred | iskeep | min | max | thin | aux), the pixel-major thin | aux copy; 0xFF everywhere the device writes
  std::vector<float> ta8((size_t)B * NPX * 8);
  for (int b = 0; b < B; ++b)
    for (int ch = 0; ch < 8; ++ch) {
      const float* src = (ch < 4 ? a->thin : a->aux) + ((size_t)b * 4 + (ch & 3)) * NPX;
      for (int p = 0; p < NPX; ++p) ta8[((size_t)b * NPX + p) * 8 + ch] = src[p];
    }
  HIPCHK(c, hipMemcpyAsync(c->l_ta8, ta8.data(), ta8.size() * 4, hipMemcpyHostToDevice, st));
  for (int b = 0; b < B; ++b) {
    float* s = d + (size_t)b * SG_STRIDE;
    HIPCHK(c, hipMemcpyAsync(s + SG_JUNCS, a->juncs_pred + (size_t)b * 600, 600 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s + SG_LP, a->lines_pred + (size_t)b * NP * 4, (size_t)NP * 16, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s + SG_THIN, a->thin + (size_t)b * 4 * NPX, (size_t)4 * NPX * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s + SG_AUX, a->aux + (size_t)b * 4 * NPX, (size_t)4 * NPX * 4, hipMemcpyHostToDevice, st));
    if (a->j2l == 0) {
      HIPCHK(c, hipMemcpyAsync(s + SG_KEEP, a->iskeep_in + (size_t)b * NP, (size_t)NP * 4, hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemcpyAsync(s + SG_MIN, a->idx_min_in + (size_t)b * NP, (size_t)NP * 4, hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemcpyAsync(s + SG_MAX, a->idx_max_in + (size_t)b * NP, (size_t)NP * 4, hipMemcpyHostToDevice, st));
    } else {
      HIPCHK(c, hipMemsetAsync(s + SG_KEEP, 0xFF, (size_t)3 * NP * 4, st));          // (iskeep | min | max are one run of the block)
    }
  }
  static_assert(SG_MIN == SG_KEEP + KEEP_CAP && SG_MAX == SG_MIN + KEEP_CAP, "iskeep | min | max are contiguous");
  const size_t L = (size_t)B;
  HIPCHK(c, hipMemsetAsync(c->wf_counts, 0xFF, L * LINE_CNT_LD * 4, st));
  HIPCHK(c, hipMemsetAsync(c->wf_keep, 0xFF, L * KEEP_CAP * 4, st));
  HIPCHK(c, hipMemsetAsync(c->wf_pairs, 0xFF, L * LINE_CAP * 8, st));
  HIPCHK(c, hipMemsetAsync(c->wf_rep, 0xFF, L * LINE_CAP * 4, st));
  HIPCHK(c, hipMemsetAsync(c->wf_prop, 0xFF, L * LINE_CAP * 16, st));
  HIPCHK(c, hipMemsetAsync(c->s1_la, 0xFF, L * LINE_CAP * 16, st));
  HIPCHK(c, hipMemsetAsync(c->s1_sc, 0xFF, L * LINE_CAP * 4, st));
  HIPCHK(c, hipMemsetAsync(c->s1_jfeat, 0xFF, L * 300 * 256 * 4, st));
  HIPCHK(c, hipMemsetAsync(c->l_ridx, 0xFF, L * 1200 * 4, st));
  // ---- line_branch_dev's match (line_match)
  c->wf_counted = false;                                     // (j2l = 0: the caller's match, which nothing has counted)
  if (a->j2l) line_match(c, B, a->j2l == 1, st);
  if (a->j2l == 2 && !c->wf_counted) { (void)hipStreamSynchronize(st); return fail(c, "debug_line_mid: the cell search did not leave the per-workgroup counts (the line path's form)"); }
  // ---- line_tail_dev: the kept list and the unique pairs (line_dedup)
  line_dedup(c, B, st);
  HIPCHK(c, hipStreamSynchronize(st));                       // (ta8 is on the device)
  if (launch_status(c)) return 1;
  HIPCHK(c, hipMemcpy(a->head4, c->s1_la, L * LINE_CAP * 16, hipMemcpyDeviceToHost));
  if (form != 3) HIPCHK(c, hipMemsetAsync(c->s1_la, 0xFF, L * LINE_CAP * 16, st));      // stage 1 of forms 0 .. 2 writes lines_adjusted itself
  // ---- the junction projections and stage 1
  std::vector<float> chw, head, lrows;                       // (staged with the stream's copies: alive until the synchronisation behind stage 1)
  if (form == 0) {
    chw.resize((size_t)128 * NPX);
    for (int p = 0; p < NPX; ++p)
      for (int ch = 0; ch < 128; ++ch) chw[(size_t)ch * NPX + p] = a->loi[(size_t)p * 128 + ch];
    HIPCHK(c, hipMemcpyAsync(c->s0_loi, chw.data(), chw.size() * 4, hipMemcpyHostToDevice, st));
  } else if (form == 1) {
    head.resize((size_t)NPX * 160);
    memset(head.data(), 0xFF, head.size() * 4);              // (columns 128 .. 159: the 17 decoded channels, which nothing behind stage 0 reads)
    for (int p = 0; p < NPX; ++p) memcpy(&head[(size_t)p * 160], a->loi + (size_t)p * 128, 128 * 4);
    HIPCHK(c, hipMemcpyAsync(c->l_head, head.data(), head.size() * 4, hipMemcpyHostToDevice, st));
  } else {
    const int M = B * 1200;
    if (line_tap_rows(c, B, st)) return 1;
    HIPCHK(c, hipStreamSynchronize(st));
    if (launch_status(c)) return 1;
    std::vector<int> ridx((size_t)M);
    HIPCHK(c, hipMemcpy(ridx.data(), c->l_ridx, ridx.size() * 4, hipMemcpyDeviceToHost));
    lrows.resize((size_t)M * 128);
    for (int r = 0; r < M; ++r) {                            // what the gather GEMM (line_loi_rows) hands on: row ridx[r] of the [B * 128*128][128] line-feature matrix
      const int b = r / 1200;
      if (ridx[r] < b * NPX || ridx[r] >= (b + 1) * NPX) return fail(c, "debug_line_mid: launch_s1_junc_rows listed a row outside its image");
      memcpy(&lrows[(size_t)r * 128], a->loi + (size_t)ridx[r] * 128, 128 * 4);
    }
    HIPCHK(c, hipMemcpyAsync(c->l_lrows, lrows.data(), lrows.size() * 4, hipMemcpyHostToDevice, st));
  }
  static_assert(S1_CHW == 0 && S1_HEAD == 1 && S1_ROWS == 2 && S1_ROWS_H == 3, "s1_form (include/airfe_debug.h) is S1Form's first four");
  line_stage1(c, B, form, a->wgs, st);
  HIPCHK(c, hipStreamSynchronize(st));
  if (launch_status(c)) return 1;
  if (saturation_status(c)) return 1;
  // ---- everything back as the device left it
  const size_t np4 = (size_t)NP * 4;
  HIPCHK(c, hipMemcpy2D(a->iskeep, np4, d + SG_KEEP, SG_STRIDE * 4, np4, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy2D(a->idx_min, np4, d + SG_MIN, SG_STRIDE * 4, np4, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy2D(a->idx_max, np4, d + SG_MAX, SG_STRIDE * 4, np4, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy2D(a->counts, 8, c->wf_counts, LINE_CNT_LD * 4, 8, B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->keep, c->wf_keep, L * KEEP_CAP * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->pairs, c->wf_pairs, L * LINE_CAP * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->rep, c->wf_rep, L * LINE_CAP * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->prop4, c->wf_prop, L * LINE_CAP * 16, hipMemcpyDeviceToHost));
  if (form >= 2) HIPCHK(c, hipMemcpy(a->ridx, c->l_ridx, L * 1200 * 4, hipMemcpyDeviceToHost));
  if (form >= 1) HIPCHK(c, hipMemcpy(a->proj, c->s1_jfeat, L * 300 * 256 * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->lines_adjusted, c->s1_la, L * LINE_CAP * 16, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->scores_line, c->s1_sc, L * LINE_CAP * 4, hipMemcpyDeviceToHost));
  std::vector<int> table(L * 300 * 300);
  HIPCHK(c, hipMemcpy(table.data(), c->wf_table, table.size() * 4, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    int dirty = 0;
    for (size_t i = 0; i < (size_t)300 * 300; ++i) dirty += table[(size_t)b * 300 * 300 + i] != 0x7FFFFFFF;
    a->table_dirty[b] = dirty;
  }
  return 0;
} AIRFE_CATCH(c)

/* the stage-0 decode (include/airfe_debug.h): line_branch_dev's steps line_decode_rows, line_head_decode, or line_head_gemm + line_decode_rows (fuse_dec = 0), on host head
 * rows / line features staged into the line branch's own buffers */
int airfe_debug_s0_decode(airfe_ctx* c, airfe_debug_s0_decode_args* a) try {
  AIRFE_ENTER(c);
  if (!c->has_s0 || !c->s0_stage || !c->l_ta8 || !c->s0_loi) return fail(c, "debug_s0_decode: the line path is not loaded (line.* tensors, cfg.plnet_s1_pack)");
  if (!a || !a->stage || !a->jloc || !a->joff || !a->jnms || !a->ta8 || !a->loi) return fail(c, "debug_s0_decode: null argument");
  const int B = a->B, mode = a->mode;
  const size_t NPX = 128 * 128;
  if (B < 1 || B > c->Lmax) return fail(c, "debug_s0_decode: 1 <= B <= the arena's images");
  if (mode < 0 || mode > 2) return fail(c, "debug_s0_decode: mode is 0 .. 2");
  if (a->stage_floats != SG_STRIDE) return fail(c, "debug_s0_decode: stage_floats is not the library's stage stride");
  if (mode == 0) {
    if (!a->rows) return fail(c, "debug_s0_decode: mode 0 needs rows");
    if (!((a->ld == 160 && a->off == 128) || (a->ld == 32 && a->off == 0))) return fail(c, "debug_s0_decode: the layouts are (ld 160, off 128) and (ld 32, off 0)");
    if (a->want_loi && a->ld != 160) return fail(c, "debug_s0_decode: the CHW loi copy exists for the (ld 160, off 128) layout only");
  } else {
    if (!a->x || !a->w || !a->b || (mode == 2 && !a->head_rows)) return fail(c, "debug_s0_decode: modes 1 and 2 need x, w and b (mode 2: head_rows)");
    if (a->prec != 0 && a->prec != 1) return fail(c, "debug_s0_decode: prec is 0 (bf16) or 1 (fp16)");
    if (a->wgs < 0 || a->wgs > 4096) return fail(c, "debug_s0_decode: wgs must lie in 0 .. 4096");
    if (a->want_loi) return fail(c, "debug_s0_decode: the CHW loi copy exists for the (ld 160, off 128) layout only");
  }
  hipStream_t st = c->stream;
  float* d = c->s0_stage;
  clear_saturation(c);
  DbgTmp t(mode ? a->prec : 0);
  float* djnms = dbg_canary<float>(&t.h, (size_t)B * NPX);
  if (!djnms) return fail(c, "debug_s0_decode: allocation failed");
  float* jnms = a->want_jnms ? djnms : nullptr;
  // ---- every output 0xFF
  HIPCHK(c, hipMemsetAsync(d, 0xFF, (size_t)B * SG_STRIDE * 4, st));
  HIPCHK(c, hipMemsetAsync(c->l_jloc, 0xFF, (size_t)B * NPX * 4, st));
  HIPCHK(c, hipMemsetAsync(c->l_joff, 0xFF, (size_t)B * 2 * NPX * 4, st));
  HIPCHK(c, hipMemsetAsync(c->l_ta8, 0xFF, (size_t)B * 8 * NPX * 4, st));
  HIPCHK(c, hipMemsetAsync(c->s0_loi, 0xFF, (size_t)128 * NPX * 4, st));
  std::vector<uint16_t> xin;                                 // (staged with the stream's copies: alive until the synchronisation behind the launches)
  if (mode == 0) {
    const size_t n = (size_t)B * NPX * a->ld;
    float* head = a->ld == 32 ? c->l_dec : c->l_head;
    if (a->ld == 160 && B > 1) {                             // (l_head holds one image)
      head = dalloc<float>(&t.h, n, false);
      if (!head) return fail(c, "debug_s0_decode: allocation failed");
    }
    HIPCHK(c, hipMemcpyAsync(head, a->rows, n * 4, hipMemcpyHostToDevice, st));
    line_decode_rows(c, B, head, a->ld, a->off, jnms, a->want_ta8 != 0, a->want_loi != 0, st);
  } else {
    const size_t n = (size_t)B * NPX * 128;
    xin.resize(n);
    for (size_t i = 0; i < n; ++i) xin[i] = cvt2(a->x[i], a->prec);
    LinW lw;
    if (!make_linear(&t.h, a->w, a->b, 128, 17, lw)) return fail(c, "debug_s0_decode: allocation failed");
    HIPCHK(c, hipMemcpyAsync(c->l_feat, xin.data(), n * 2, hipMemcpyHostToDevice, st));
    if (mode == 1) {
      line_head_decode(c, B, a->prec, lw, jnms, a->wgs, st);
    } else {                                                 // (fuse_dec = 0: the 17-channel head as a GEMM, then the decode over its rows)
      HIPCHK(c, hipMemsetAsync(c->l_dec, 0xFF, (size_t)B * NPX * 32 * 4, st));
      line_head_gemm(c, B, false, a->prec, lw, st);
      line_decode_rows(c, B, c->l_dec, 32, 0, jnms, true, false, st);
    }
  }
  HIPCHK(c, hipStreamSynchronize(st));                       // (xin goes out of scope)
  if (launch_status(c)) return 1;
  if (saturation_status(c)) return 1;
  // ---- everything back as the device left it
  HIPCHK(c, hipMemcpy(a->stage, d, (size_t)B * SG_STRIDE * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->jloc, c->l_jloc, (size_t)B * NPX * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->joff, c->l_joff, (size_t)B * 2 * NPX * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->jnms, djnms, (size_t)B * NPX * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->ta8, c->l_ta8, (size_t)B * 8 * NPX * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(a->loi, c->s0_loi, (size_t)128 * NPX * 4, hipMemcpyDeviceToHost));
  if (mode == 2) HIPCHK(c, hipMemcpy(a->head_rows, c->l_dec, (size_t)B * NPX * 32 * 4, hipMemcpyDeviceToHost));
  c->wf_counted = false;                                     // (the stage blocks no longer hold a line branch's match)
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_junctions_topk(airfe_ctx* c, const float* jloc, const float* joff, int B, float* juncs_pred) try {
  AIRFE_ENTER(c);
  if (!c->has_s0 || !c->s0_stage) return fail(c, "debug_junctions_topk: the line branch is not loaded (line.* tensors, cfg.plnet_s1_pack)");
  if (!jloc || !joff || !juncs_pred || B < 1 || B > c->Lmax) return fail(c, "debug_junctions_topk: bad argument (1 <= B <= the arena's images)");
  const size_t npx = 128 * 128;
  hipStream_t st = c->stream;
  clear_saturation(c);
  HIPCHK(c, hipMemcpyAsync(c->l_jloc, jloc, (size_t)B * npx * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->l_joff, joff, (size_t)B * 2 * npx * 4, hipMemcpyHostToDevice, st));
  junctions_topk_dev(c, B, st);
  HIPCHK(c, hipStreamSynchronize(st));
  if (launch_status(c)) return 1;
  if (saturation_status(c)) return 1;
  HIPCHK(c, hipMemcpy2D(juncs_pred, 600 * 4, c->s0_stage + SG_JUNCS, SG_STRIDE * 4, 600 * 4, B, hipMemcpyDeviceToHost));
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_detector_maps(airfe_ctx* c, int B, float* heat_raw, float* heat_nms, float* desc) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_sp || B > c->Dmax) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t R = AIRFE_INTERNAL_SIZE;
  if (heat_raw) HIPCHK(c, hipMemcpy(heat_raw, c->heat, (size_t)B * R * R * 4, hipMemcpyDeviceToHost));
  if (heat_nms && c->cfg.nms_radius > 0 && !c->nms_map_valid) {      // the batch path skipped the dense map: rebuild it from the heat maps
    launch_nms512_candidates(c->heat, c->heat_nms, c->nms_mask, (int)B, c->cfg.keypoint_threshold, c->cfg.remove_borders, c->cand, c->cand_cnt,
                             R * R, c->stream);          // (the map is only ever skipped on the radius-4 path)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->nms_map_valid = true;
  }
  if (heat_nms) HIPCHK(c, hipMemcpy(heat_nms, c->cfg.nms_radius > 0 ? c->heat_nms : c->heat, (size_t)B * R * R * 4, hipMemcpyDeviceToHost));
  if (desc) {
    if (!c->desc_dense_valid) {     // the batch path ran the head on the sampled cells only: build the dense map from the kept activations
      dense_desc_head(c, c->last_B, c->stream);
      c->desc_dense_valid = true;
    }
    if (!c->desc_normalised) {      // the inspection hook returns the map the reference would hold: normalised
      launch_l2norm256(c->desc, c->Dmax * 64 * 64, c->stream);
      HIPCHK(c, hipStreamSynchronize(c->stream));
      c->desc_normalised = true;
    }
    HIPCHK(c, hipMemcpy(desc, c->desc, (size_t)B * 64 * 64 * 256 * 4, hipMemcpyDeviceToHost));
  }
  return 0;
} AIRFE_CATCH(c)

/* the on-device stage-0 line branch of the LAST detected image, copied out in the Appendix A.1 layouts (NULL = skip) */
int airfe_debug_plnet_stage0(airfe_ctx* c, float* juncs_pred, float* lines_pred, float* iskeep, float* idx_min, float* idx_max,
                             float* loi, float* thin, float* aux, float* jloc, float* joff) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_s0 || !c->has_s1) return fail(c, "debug_plnet_stage0: line branch / stage 1 not loaded");
  hipStream_t st = c->stream;
  if (line_branch_dev(c, st, 0, 1, true)) return 1;
  HIPCHK(c, hipStreamSynchronize(st));
  const size_t NP = KEEP_CAP;
  float* d = c->s0_stage;
  struct { float* h; const float* dv; size_t n; } cp[10] = {
      {juncs_pred, d + SG_JUNCS, 600}, {lines_pred, d + SG_LP, NP * 4}, {iskeep, d + SG_KEEP, NP}, {idx_min, d + SG_MIN, NP},
      {idx_max, d + SG_MAX, NP}, {loi, c->s0_loi, (size_t)128 * 128 * 128}, {thin, d + SG_THIN, (size_t)4 * 128 * 128},
      {aux, d + SG_AUX, (size_t)4 * 128 * 128}, {jloc, c->l_jloc, (size_t)128 * 128}, {joff, c->l_joff, (size_t)2 * 128 * 128}};
  for (auto& e : cp)
    if (e.h) HIPCHK(c, hipMemcpy(e.h, e.dv, e.n * 4, hipMemcpyDeviceToHost));
  return 0;
} AIRFE_CATCH(c)

/* the junction-to-line match of the LAST detected image as the line path runs it (fast = 1: cell search, exact where it is consumed) or
   as the inspection hook exports it (fast = 0: every proposal against every junction): iskeep, idx_junc_to_end_min / _max [3*128*128] */
int airfe_debug_plnet_j2l(airfe_ctx* c, int fast, float* iskeep, float* idx_min, float* idx_max) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_s0 || !c->has_s1) return fail(c, "debug_plnet_j2l: line branch / stage 1 not loaded");
  hipStream_t st = c->stream;
  if (line_branch_dev(c, st, 0, 1, fast == 0)) return 1;
  HIPCHK(c, hipStreamSynchronize(st));
  const size_t NP = KEEP_CAP;
  float* d = c->s0_stage;
  if (iskeep) HIPCHK(c, hipMemcpy(iskeep, d + SG_KEEP, NP * 4, hipMemcpyDeviceToHost));
  if (idx_min) HIPCHK(c, hipMemcpy(idx_min, d + SG_MIN, NP * 4, hipMemcpyDeviceToHost));
  if (idx_max) HIPCHK(c, hipMemcpy(idx_max, d + SG_MAX, NP * 4, hipMemcpyDeviceToHost));
  return 0;
} AIRFE_CATCH(c)

/* stage-1 alone on HOST stage-0 tensors: lines_adjusted [M2][4] + scores_line [M2] (parity vs the real plnet_s1.onnx) */
int airfe_debug_plnet_s1(airfe_ctx* c, const airfe_plnet_stage0* s0, float* lines_adjusted, float* scores_line, int cap, int* m2) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_s1 || !s0) return fail(c, "debug_plnet_s1: stage-1 not loaded");
  hipStream_t st = c->stream;
  if (upload_stage0(c, s0, st)) return 1;
  line_dedup(c, 1, st);                        // (upload_stage0 left wf_counted false: host tensors, nothing has counted their kept proposals)
  line_stage1(c, 1, S1_CHW, 0, st);
  int cnt[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(cnt, c->wf_counts, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int k = std::min(cnt[1], cap);
  if (k > 0) {
    HIPCHK(c, hipMemcpy(lines_adjusted, c->s1_la, (size_t)k * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(scores_line, c->s1_sc, (size_t)k * 4, hipMemcpyDeviceToHost));
  }
  *m2 = k;
  return 0;
} AIRFE_CATCH(c)

int airfe_debug_plnet_s1_last(airfe_ctx* c, float* lines_adjusted, float* scores_line, int cap, int* m2) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_s1 || !lines_adjusted || !scores_line || !m2) return fail(c, "debug_plnet_s1_last: stage-1 not loaded / bad argument");
  HIPCHK(c, hipDeviceSynchronize());
  int cnt[2] = {0, 0};
  HIPCHK(c, hipMemcpy(cnt, c->wf_counts, 8, hipMemcpyDeviceToHost));
  const int k = std::min(cnt[1], cap);
  if (k > 0) {
    HIPCHK(c, hipMemcpy(lines_adjusted, c->s1_la, (size_t)k * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(scores_line, c->s1_sc, (size_t)k * 4, hipMemcpyDeviceToHost));
  }
  *m2 = k;
  return 0;
} AIRFE_CATCH(c)

}  // extern "C"
