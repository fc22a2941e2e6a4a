// airfe — the kernel-level test hooks of libairfe.so (include/airfe_debug.h): host tensors -> one production launcher or line-path step -> host tensors.  Every hook has one
// shape: argument checks, staging through a HookStage, the launches, the wait, read-backs through the HookStage.
#include "airfe_host.h"
#include "wg_prims.h"

#include <limits.h>
#include <memory>

// One hook call's device work, bound to the context, the hook's name and the context's stream: every buffer the hook makes, every fill, upload and read-back, and the wait.
//  * A device write made before the launches is complete when the call that made it returns (make_linear's blocking copies) or is queued on the stream the launches go to;
//    nothing is queued on the null stream, which that (non-blocking) stream would not wait for, and nothing waits for it.
//  * The host side of every queued copy is kept here until the holder dies.
//  * After the first failure every later operation does nothing; the hook returns status().
//  * The destructor waits for the stream when work was queued and not waited for, then frees: on every way out, an exception caught by AIRFE_CATCH included.
struct HookStage {
  enum { OWN_TEXT = 1, SATURATION = 2, DEVICE_WIDE = 4 };                  // wait(): "<hook>: kernel failed" for a failed wait or launch | saturation_status too | the whole device
  HookStage(airfe_ctx* c_, const std::string& who_, int pack_prec = 0) : c(c_), who(who_), st(c_->stream) { mem.pack_prec = pack_prec; }
  HookStage(const HookStage&) = delete;
  ~HookStage() {
    if (queued) (void)hipStreamSynchronize(st);
    for (void* p : mem.allocs) (void)hipFree(p);
  }
  int status() const { return rc; }
  hipStream_t stream() { queued = true; return st; }                       // for the hook's launches: whoever takes the stream queues on it
  int refuse(const std::string& m) { return rc ? rc : rc = fail(c, who + ": " + m); }
  void step(int r) { queued = true; if (r) rc = 1; }                       // a production step's own status (it has set the context's error)
  template <class T> T* fresh(size_t n, int byte) {                        // a new buffer whose every byte is `byte` (0x00, or 0xFF: NaN in fp32, fp16 and bf16) when the launches start
    T* p = raw<T>(n);
    fill(p, byte, std::max<size_t>(n, 1) * sizeof(T));
    return p;
  }
  template <class T> T* up(std::vector<T> v) { T* p = raw<T>(v.size()); put(p, std::move(v)); return p; }      // a new buffer holding v
  template <class T> T* up(const T* src, size_t n) { return up(std::vector<T>(src, src + n)); }
  bool linear(const float* W, const float* b, int K, int N, LinW& out) { if (!rc && !make_linear(&mem, W, b, K, N, out)) refuse("allocation failed"); return !rc; }
  // the same two on memory the context owns (the arena and line-path buffers a hook stages into and restores)
  void fill(void* p, int byte, size_t bytes) { if (!rc && bytes) hip(hipMemsetAsync(p, byte, bytes, stream()), "hipMemsetAsync"); }
  template <class T> void put(void* dst, std::vector<T> v) {
    auto h = std::make_shared<std::vector<T>>(std::move(v));
    host.push_back(h);
    if (!rc && !h->empty()) hip(hipMemcpyAsync(dst, h->data(), h->size() * sizeof(T), hipMemcpyHostToDevice, stream()), "hipMemcpyAsync");
  }
  void put(void* dst, const void* src, size_t bytes) { put2d(dst, bytes, src, bytes, bytes, 1); }
  void put2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {      // the host rows are kept packed
    std::vector<uint8_t> v(width * rows);
    for (size_t r = 0; r < rows; ++r) memcpy(v.data() + r * width, static_cast<const uint8_t*>(src) + r * spitch, width);
    if (rows == 1 || dpitch == width) return put(dst, std::move(v));
    auto h = std::make_shared<std::vector<uint8_t>>(std::move(v));
    host.push_back(h);
    if (!rc && !h->empty()) hip(hipMemcpy2DAsync(dst, dpitch, h->data(), width, width, rows, hipMemcpyHostToDevice, stream()), "hipMemcpy2DAsync");
  }
  int wait(unsigned how = 0) {                                             // the stream idle, then launch_status, then (SATURATION) saturation_status
    if (rc) return rc;
    const hipError_t e = (how & DEVICE_WIDE) ? hipDeviceSynchronize() : hipStreamSynchronize(st);
    queued = false;
    if (how & OWN_TEXT) { if (e != hipSuccess || launch_status(c)) refuse("kernel failed"); }
    else if (hip(e, (how & DEVICE_WIDE) ? "hipDeviceSynchronize" : "hipStreamSynchronize") && launch_status(c)) rc = 1;
    if (!rc && (how & SATURATION) && saturation_status(c)) rc = 1;
    return rc;
  }
  // read-backs, after the wait: blocking, checked
  void get(void* dst, const void* src, size_t bytes) { if (!rc && bytes) hip(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "hipMemcpy"); }
  template <class T> std::vector<T> get(const void* src, size_t n) { std::vector<T> v(n); get(v.data(), src, n * sizeof(T)); return v; }
  void get2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    if (!rc && width && rows) hip(hipMemcpy2D(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToHost), "hipMemcpy2D");
  }

 private:
  airfe_ctx* c; std::string who; hipStream_t st;
  DevAllocs mem;                                                           // what dalloc / dupload / make_linear read of a context, owned here
  std::vector<std::shared_ptr<void>> host;
  int rc = 0; bool queued = false;
  bool hip(hipError_t e, const char* call) { if (e != hipSuccess) refuse(std::string(call) + ": " + hipGetErrorString(e)); return e == hipSuccess; }
  template <class T> T* raw(size_t n) {
    void* p = nullptr;
    if (rc) return nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) { refuse("allocation failed"); return nullptr; }
    mem.allocs.push_back(p);
    return static_cast<T*>(p);
  }
};
struct DevSpan { void* p; size_t bytes; };                                 // for "every output 0xFF when the launch starts" / "zero again when the hook returns"

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
// the GEMM family's staging: rows padded with zero rows to rows_cap
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
static void dbg_back2(const std::vector<uint16_t>& v, size_t n, int prec, float* out) {
  for (size_t i = 0; i < n; ++i) out[i] = back2(v[i], prec);
}
static void dbg_gemm_dispatch(const airfe_ctx* c, GemmArgs& g, int gr_wgs) {      // the context's dispatch thresholds, as run_linear hands them on
  g.small_max = c->gemm_small_max; g.g8_min = c->gemm8_min; g.gr_min = c->gemmr_min; g.gr_wgs = gr_wgs > 0 ? gr_wgs : c->gemmr_wgs;
}

// wg_prims.h on host arrays (airfe_debug_wg_prims): one workgroup, rounds of THREADS with a running base as in the production loops
template <int THREADS, class K>
__global__ __launch_bounds__(THREADS) void wg_prims_kernel(const int* v, const uint8_t* keep, int n, const K* keys, int P, int* scan, int* pos, int* totals, int* wave,
                                                           K* sorted) {
  __shared__ int wsum[THREADS / 64];
  __shared__ K key[32768 / sizeof(K)];
  const int t = threadIdx.x;
  const int x0 = t < n ? v[t] : 0;
  const int ws = wave_sum(x0), wx = wave_max(x0), wn = wave_min(x0);
  if ((t & 63) == 0) { wave[3 * (t >> 6)] = ws; wave[3 * (t >> 6) + 1] = wx; wave[3 * (t >> 6) + 2] = wn; }
  int sbase = 0, cbase = 0, s = 0, mx = INT_MIN, mn = INT_MAX;
  for (int i0 = 0; i0 < n; i0 += THREADS) {                    // (uniform)
    const int i = i0 + t;
    const int x = i < n ? v[i] : 0;
    int stot, ctot;
    const int ex = sbase + block_excl_scan<THREADS>(x, wsum, &stot);
    const int p = cbase + block_compact<THREADS>(i < n && keep[i], wsum, &ctot);
    if (i < n) { scan[i] = ex; pos[i] = p; s += x; mx = max(mx, x); mn = min(mn, x); }
    sbase += stot;
    cbase += ctot;
  }
  s = block_sum<THREADS>(s, wsum);
  mx = block_max<THREADS>(mx, wsum);
  mn = block_min<THREADS>(mn, wsum);
  if (t == 0) { totals[0] = sbase; totals[1] = cbase; totals[2] = s; totals[3] = mx; totals[4] = mn; }
  for (int i = t; i < P; i += THREADS) key[i] = keys[i];
  block_sort_asc<THREADS>(key, P);
  for (int i = t; i < P; i += THREADS) sorted[i] = key[i];
}
template <int THREADS>
static void launch_wg_prims(const airfe_debug_wg_prims_args* a, const int* v, const uint8_t* keep, const void* keys, int* out, void* sorted, hipStream_t st) {
  int *scan = out, *pos = out + a->n, *totals = out + 2 * a->n, *wave = totals + 5;
  if (a->key_bytes == 4)
    hipLaunchKernelGGL((wg_prims_kernel<THREADS, unsigned>), dim3(1), dim3(THREADS), 0, st, v, keep, a->n, static_cast<const unsigned*>(keys), a->P, scan, pos, totals,
                       wave, static_cast<unsigned*>(sorted));
  else
    hipLaunchKernelGGL((wg_prims_kernel<THREADS, unsigned long long>), dim3(1), dim3(THREADS), 0, st, v, keep, a->n, static_cast<const unsigned long long*>(keys), a->P,
                       scan, pos, totals, wave, static_cast<unsigned long long*>(sorted));
}

extern "C" {

// ---- kernel-level test hooks ------------------------------------------------------------------------------
int airfe_debug_preprocess(airfe_ctx* c, const uint8_t* gray, int h, int w, int stride, float* out) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_sp) return fail(c, "debug_preprocess: detector not loaded");
  const size_t bytes = (size_t)h * stride;
  const int R = AIRFE_INTERNAL_SIZE;
  HookStage s(c, "debug_preprocess");
  s.step(upload_image(c, gray, h, w, stride) || ensure_tables(c, h, w));
  if (s.status()) return 1;
  launch_preprocess(c->st_img.p, 1, h, w, stride, bytes, c->xtab, c->ytab, c->lut, c->img32, R, R, s.stream());
  s.wait();
  s.get2d(out, (size_t)R * 4, c->img32 + (R + 2) + 1, (size_t)(R + 2) * 4, (size_t)R * 4, R);
  return s.status();
} AIRFE_CATCH(c)

int airfe_debug_conv3x3(airfe_ctx* c, const float* x, int B, int cin, int H, int W, const float* w, const float* b, int cout,
                        int pool, float* y) try {
  AIRFE_ENTER(c);
  if ((cin != 64 && cin != 128) || cout % 64 || W % 16 || H % 16) return fail(c, "debug_conv3x3: unsupported shape");
  const int prec = c->prec;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  const size_t ywords = (size_t)B * (Ho + 2) * (Wo + 2) * cout;
  HookStage s(c, "debug_conv3x3");
  ConvArgs a;
  a.X = s.up(dbg_conv_x(x, B, cin, H, W, prec)); a.Wp = s.up(dbg_conv_slabs(w, cin, cout, prec));
  a.bias = s.up(b, (size_t)cout); a.Y = s.fresh<uint16_t>(ywords, 0);
  a.B = B; a.H = H; a.W = W; a.CIN = cin; a.COUT = cout;
  a.pool = pool; a.out_pad = 1; a.relu = 1;
  if (s.status()) return 1;
  launch_conv3x3(prec, a, s.stream());
  s.wait();
  const std::vector<uint16_t> yo = s.get<uint16_t>(a.Y, ywords);
  for (int bb = 0; bb < B; ++bb)
    for (int co = 0; co < cout; ++co)
      for (int yy = 0; yy < Ho; ++yy)
        for (int xx = 0; xx < Wo; ++xx)
          y[(((size_t)bb * cout + co) * Ho + yy) * Wo + xx] = back2(yo[(((size_t)bb * (Ho + 2) + yy + 1) * (Wo + 2) + xx + 1) * cout + co], prec);
  return s.status();
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
  HookStage s(c, "debug_gemm", prec);
  LinW lw;
  s.linear(w, b, K, N, lw);
  GemmArgs g;
  g.X1 = s.up(dbg_rows2(x, M, K, Mp, prec)); g.ld1 = K; g.K1 = K; g.Wp = lw.w; g.bias = lw.b; g.M = Mp; g.N = N; g.cb_total = lw.cbt;
  g.epi = EPI_STORE_F32; g.act = relu ? ACT_RELU : ACT_NONE; g.out = s.fresh<float>((size_t)Mp * Np8, 0); g.ldo = Np8;
  dbg_gemm_dispatch(c, g, 0);
  if (s.status()) return 1;
  launch_gemm(prec, K, false, g, s.stream());
  s.wait(HookStage::OWN_TEXT);
  const std::vector<float> yo = s.get<float>(g.out, (size_t)Mp * Np8);
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) y[(size_t)m * N + n] = yo[(size_t)m * Np8 + n];
  return s.status();
} AIRFE_CATCH(c)

// ---- the GEMM family one form at a time (include/airfe_debug.h): host tensors -> the production launchers -> host tensors
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
  HookStage s(c, "debug_conv");
  ConvArgs g;
  if (fused) {
    std::vector<float> im((size_t)B * (H + 2) * (W + 2), 0.f);
    for (int bb = 0; bb < B; ++bb)
      for (int yy = 0; yy < H; ++yy) memcpy(&im[((size_t)bb * (H + 2) + yy + 1) * (W + 2) + 1], a->img + ((size_t)bb * H + yy) * W, (size_t)W * sizeof(float));
    g.img = s.up(std::move(im));
    g.w1a = s.up(a->w1a, (size_t)64 * 9);
    g.b1a = s.up(a->b1a, (size_t)64);
  } else {
    g.X = s.up(dbg_conv_x(a->x, B, cin, H, W, prec));
  }
  g.Wp = s.up(dbg_conv_slabs(a->w, cin, cout, prec));
  g.bias = s.up(a->b, (size_t)cout);
  uint16_t* dy = s.fresh<uint16_t>(total, 0xFF);
  if (s.status()) return 1;
  g.Y = dy + guard;
  g.B = B; g.H = H; g.W = W; g.CIN = cin; g.COUT = cout; g.pool = pool; g.out_pad = opad; g.relu = a->relu; g.wgs = a->wgs;
  if (fused) launch_conv64r(prec, g, s.stream());        // as detect_dev2 launches the first layer
  else launch_conv3x3(prec, g, s.stream());              // production's dispatch: conv64r / conv128r, or conv3x3_kernel for relu = 0
  s.wait(HookStage::OWN_TEXT);
  s.get(a->y_raw, dy, total * 2);
  return s.status();
} AIRFE_CATCH(c)

int airfe_debug_conv_order(int order, int* previous) try {
  if (order < -1 || order > CONV_ORDER_DEFAULT) return fail(nullptr, "debug_conv_order: order must lie in -1 .. 3");
  const int before = conv_tile_order_switch(order);
  if (previous) *previous = before;
  return 0;
} AIRFE_CATCH(nullptr)

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
  const bool f32 = epi == EPI_STORE_F32 || d2s, two = epi == EPI_HEADS && N == 512;
  const size_t out_elems = d2s ? (size_t)M * 64 : heads ? (size_t)Sg * 4 * a->Np * 64 : (size_t)Mp * ldo, out_bytes = out_elems * (f32 ? 4 : 2);
  HookStage s(c, "debug_linear", prec);
  LinW lw;
  s.linear(a->w, a->b, K, N, lw);
  GemmArgs g;
  g.X1 = s.up(dbg_rows2(a->x1, a->rowidx ? a->src_rows : M, K1, xrows, prec)); g.ld1 = K1; g.K1 = K1;
  if (a->x2) { g.X2 = s.up(dbg_rows2(a->x2, M, K - K1, Mp, prec)); g.ld2 = K - K1; }
  g.Wp = lw.w; g.bias = lw.b; g.M = Mp; g.N = N; g.cb_total = lw.cbt; g.epi = epi; g.act = a->act; g.ldo = ldo; g.Np = a->Np; g.H = 4;
  dbg_gemm_dispatch(c, g, a->gr_wgs);
  if (a->rot_cos) { g.rot_cos = s.up(dbg_rows4(a->rot_cos, M, 32, Mp)); g.rot_sin = s.up(dbg_rows4(a->rot_sin, M, 32, Mp)); }
  if (a->rowidx) { std::vector<int> ri(Mp, 0); memcpy(ri.data(), a->rowidx, (size_t)M * sizeof(int)); g.rowidx = s.up(std::move(ri)); }
  g.out = s.fresh<uint8_t>(out_bytes, 0xFF);
  if (two) g.out2 = s.fresh<uint8_t>(out_bytes, 0xFF);
  if (epi == EPI_RESID) g.x32 = s.up(dbg_rows4(a->x32, M, N, Mp));
  if (d2s) { g.d2s_hc = a->d2s_hc; g.d2s_wc = a->d2s_wc; g.flag = s.fresh<int>(1, 0); }
  if (s.status()) return 1;
  // a forced kernel runs only where its own applicability test says yes: never a silent fall-back to another kernel
  const char* refused = nullptr;
  hipStream_t st = s.stream();
  switch (kern) {
    case AIRFE_DEBUG_KERNEL_DISPATCH:
      if (d2s) launch_gemm8(prec, K, false, g, st);
      else launch_gemm(prec, K, trans, g, st);
      break;
    case AIRFE_DEBUG_KERNEL_SMALL:                       // launch_gemm's own row test with every other path moved out of reach
      if (d2s || a->rowidx) refused = "gemm_small";
      else { g.small_max = 1 << 30; g.g8_min = 1 << 30; g.gr_min = 1 << 30; launch_gemm(prec, K, trans, g, st); }
      break;
    case AIRFE_DEBUG_KERNEL_TILED:
      if (d2s || a->rowidx || K1 % 64) refused = "gemm_kernel";
      else { g.small_max = -1; g.g8_min = 1 << 30; g.gr_min = 1 << 30; launch_gemm(prec, K, trans, g, st); }
      break;
    case AIRFE_DEBUG_KERNEL_GEMM8:
      if (K1 % 64) refused = "gemm8";
      else launch_gemm8(prec, K, trans, g, st);
      break;
    case AIRFE_DEBUG_KERNEL_GEMMR:
      if (a->rowidx || !gemmr_applicable(K, trans, g)) refused = "gemmr";
      else launch_gemmr(prec, trans, g, st);
      break;
    case AIRFE_DEBUG_KERNEL_GEMMR_GATHER:
      if (!gemmr_gather_applicable(K, g)) refused = "gemmr_gather";
      else launch_gemmr_gather(prec, g, st);
      break;
    default:
      if (!gemmr_gather128_applicable(g)) refused = "gemmr_gather128";
      else launch_gemmr_gather128(prec, g, st);
      break;
  }
  if (refused) return s.refuse(std::string(refused) + " does not apply to this form");
  s.wait(HookStage::OWN_TEXT);
  if (f32) {
    const std::vector<float> ho = s.get<float>(g.out, out_elems);
    for (int m = 0; m < (d2s ? 1 : M); ++m) memcpy(a->out + (size_t)m * N, ho.data() + (size_t)m * ldo, (d2s ? out_elems : (size_t)N) * 4);
    if (d2s && a->flag) s.get(a->flag, g.flag, sizeof(int));
  } else if (heads) {
    const size_t n = (size_t)S * 4 * a->Np * 64;
    dbg_back2(s.get<uint16_t>(g.out, out_elems), n, prec, a->out);
    if (two) dbg_back2(s.get<uint16_t>(g.out2, out_elems), n, prec, a->out2);
  } else {
    const std::vector<uint16_t> ho = s.get<uint16_t>(g.out, out_elems);
    for (int m = 0; m < M; ++m)
      for (int n = 0; n < N; ++n) a->out[(size_t)m * N + n] = back2(ho[(size_t)m * ldo + n], prec);
    if (epi == EPI_RESID) s.get(a->x32, g.x32, (size_t)M * N * 4);
  }
  return s.status();
} AIRFE_CATCH(c)

int airfe_debug_qkv(airfe_ctx* c, int prec, int M, int Np, const float* x, const float* wqk, const float* bqk, int nqk, const float* wv, const float* bv,
                    const float* rot_cos, const float* rot_sin, int pair, int gr_wgs, float* q, float* k, float* vt) try {
  AIRFE_ENTER(c);
  if ((prec != 0 && prec != 1) || M < 1 || Np < 16 || Np % 16 || M % Np || (nqk != 256 && nqk != 512) || !x || !wqk || !bqk || !wv || !bv || !q || !vt ||
      (nqk == 512 && !k) || (!rot_cos) != (!rot_sin))
    return fail(c, "debug_qkv: bad argument");
  const int Mp = (M + 127) / 128 * 128, Sg = (Mp + Np - 1) / Np, S = M / Np;
  const size_t elems = (size_t)Sg * 4 * Np * 64, n = (size_t)S * 4 * Np * 64;
  HookStage s(c, "debug_qkv", prec);
  LinW lqk, lv;
  s.linear(wqk, bqk, 256, nqk, lqk);
  s.linear(wv, bv, 256, 256, lv);
  GemmArgs ga, gb;
  ga.X1 = gb.X1 = s.up(dbg_rows2(x, M, 256, Mp, prec));
  ga.ld1 = gb.ld1 = 256; ga.K1 = gb.K1 = 256; ga.M = gb.M = Mp; ga.Np = gb.Np = Np; ga.H = gb.H = 4;
  ga.Wp = lqk.w; ga.bias = lqk.b; ga.N = nqk; ga.cb_total = lqk.cbt; ga.epi = EPI_HEADS; ga.ldo = nqk;
  gb.Wp = lv.w; gb.bias = lv.b; gb.N = 256; gb.cb_total = lv.cbt; gb.epi = EPI_HEADS_T; gb.ldo = 256;
  ga.out = s.fresh<uint16_t>(elems, 0xFF);
  if (nqk == 512) ga.out2 = s.fresh<uint16_t>(elems, 0xFF);
  gb.out = s.fresh<uint16_t>(elems, 0xFF);
  if (rot_cos) { ga.rot_cos = s.up(dbg_rows4(rot_cos, M, 32, Mp)); ga.rot_sin = s.up(dbg_rows4(rot_sin, M, 32, Mp)); }
  dbg_gemm_dispatch(c, ga, gr_wgs);
  dbg_gemm_dispatch(c, gb, gr_wgs);
  if (s.status()) return 1;
  if (pair) {
    if (!gemmr_pair_applicable(ga, gb)) return s.refuse("gemmr_pair does not apply to this form");
    launch_gemmr_pair(prec, ga, gb, s.stream());
  } else {
    launch_gemm(prec, 256, false, ga, s.stream());
    launch_gemm(prec, 256, true, gb, s.stream());
  }
  s.wait(HookStage::OWN_TEXT);
  dbg_back2(s.get<uint16_t>(ga.out, elems), n, prec, q);
  if (nqk == 512) dbg_back2(s.get<uint16_t>(ga.out2, elems), n, prec, k);
  dbg_back2(s.get<uint16_t>(gb.out, elems), n, prec, vt);
  return s.status();
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
  HookStage s(c, "debug_lg_block", prec);
  LinW lo, l1, l2, lq, lv;
  if (a->wo) s.linear(a->wo, a->bo, 256, 256, lo);
  s.linear(a->w1, a->b1, 512, 512, l1);
  s.linear(a->w2, a->b2, 512, 256, l2);
  if (nq) { s.linear(a->nqk_w, a->nqk_b, 256, nq, lq); s.linear(a->nv_w, a->nv_b, 256, 256, lv); }
  const bool fr = lg_blockf_frag_weights();
  const std::vector<float> x32h = dbg_rows4(a->x32, M, 256, cap);
  std::vector<uint16_t> xbh((size_t)cap * 256);
  for (size_t i = 0; i < xbh.size(); ++i) xbh[i] = cvt2(x32h[i], prec);
  std::vector<float> gb(1024, 0.f);
  if (!a->relu) { memcpy(gb.data(), a->gamma, 512 * 4); memcpy(gb.data() + 512, a->beta, 512 * 4); }
  LgBlockFArgs g;
  g.attn = s.up(dbg_rows2(a->attn, M, 256, cap, prec));
  g.xb = s.up(xbh);
  g.x32 = s.up(x32h);
  const float* dgb = s.up(std::move(gb));
  g.gamma = dgb; g.beta = dgb ? dgb + 512 : nullptr;
  g.wo = a->wo ? (fr ? lo.wf : lo.w) : nullptr; g.bo = a->wo ? lo.b : nullptr;
  g.w1 = fr ? l1.wf : l1.w; g.b1 = l1.b; g.w2 = fr ? l2.wf : l2.w; g.b2 = l2.b;
  g.M = M; g.tokens_per_wg = T; g.mixed = a->mixed; g.n_cu = c->n_cu; g.relu = a->relu;
  if (nq) {
    g.nqk_w = fr ? lq.wf : lq.w; g.nqk_b = lq.b; g.nqk_n = nq; g.nv_w = fr ? lv.wf : lv.w; g.nv_b = lv.b; g.Np = Np; g.H = 4;
    if (nq == 512) { g.rot_cos = s.up(dbg_rows4(a->rot_cos, M, 32, cap)); g.rot_sin = s.up(dbg_rows4(a->rot_sin, M, 32, cap)); }
    g.q_out = s.fresh<uint16_t>(helems, 0xFF);
    if (nq == 512) g.k_out = s.fresh<uint16_t>(helems, 0xFF);
    g.vt_out = s.fresh<uint16_t>(helems, 0xFF);
  }
  if (s.status()) return 1;
  launch_lg_blockf(prec, g, s.stream());
  s.wait(HookStage::OWN_TEXT);
  // rows past M that the launch changed: x32 / xb against their initial (zero) rows, q / k / v^T against the 0xFFFF fill
  const std::vector<float> x32o = s.get<float>(g.x32, (size_t)cap * 256);
  const std::vector<uint16_t> xbo = s.get<uint16_t>(g.xb, (size_t)cap * 256);
  memcpy(a->x32, x32o.data(), (size_t)M * 256 * 4);
  dbg_back2(xbo, (size_t)M * 256, prec, a->xb);
  for (int i = 0; i < 5; ++i) a->rows_past[i] = 0;
  for (int r = M; r < cap; ++r)
    for (int f = 0; f < 256; ++f) {
      const size_t e = (size_t)r * 256 + f;
      if (memcmp(&x32o[e], &x32h[e], 4)) a->rows_past[0] = r - M + 1;
      if (xbo[e] != xbh[e]) a->rows_past[1] = r - M + 1;
    }
  uint16_t* dev[3] = {g.q_out, g.k_out, g.vt_out};
  float* host[3] = {a->q, a->k, a->vt};
  for (int j = 0; j < 3 && nq; ++j) {
    if (!dev[j]) continue;
    const std::vector<uint16_t> ho = s.get<uint16_t>(dev[j], helems);
    dbg_back2(ho, (size_t)S * 4 * Np * 64, prec, host[j]);
    for (size_t e = (size_t)S * 4 * Np * 64; e < helems; ++e) {
      if (ho[e] == 0xFFFF) continue;
      const size_t sq = e / ((size_t)4 * Np * 64), w = e % ((size_t)Np * 64);
      const int row = (int)(sq * Np + (j == 2 ? w % Np : w / 64));          // q / k [s][h][n][64], v^T [s][h][d][n]
      a->rows_past[2 + j] = std::max(a->rows_past[2 + j], row - M + 1);
    }
  }
  return s.status();
} AIRFE_CATCH(c)

int airfe_debug_ln_gelu(airfe_ctx* c, int prec, float* h, const float* gamma, const float* beta, int M) try {
  AIRFE_ENTER(c);
  if ((prec != 0 && prec != 1) || M < 1 || !h || !gamma || !beta) return fail(c, "debug_ln_gelu: bad argument");
  HookStage s(c, "debug_ln_gelu");
  std::vector<float> gb(1024);
  memcpy(gb.data(), gamma, 512 * 4);
  memcpy(gb.data() + 512, beta, 512 * 4);
  uint16_t* dh = s.up(dbg_rows2(h, M, 512, M, prec));
  const float* dgb = s.up(std::move(gb));
  if (s.status()) return 1;
  launch_ln_gelu(prec, dh, dgb, dgb + 512, M, s.stream());
  s.wait(HookStage::OWN_TEXT);
  dbg_back2(s.get<uint16_t>(dh, (size_t)M * 512), (size_t)M * 512, prec, h);
  return s.status();
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
  HookStage s(c, who);
  const uint16_t *dq = s.up(std::move(hq)), *dk = s.up(std::move(hk)), *dv = s.up(std::move(hvt));
  const size_t out_n = (size_t)S * Np * H * 64, slack_n = (size_t)128 * H * 64;
  uint16_t* dout = s.fresh<uint16_t>(out_n + slack_n, a->canary ? 0xFF : 0);
  const int* dl = s.up(a->lens, (size_t)S);
  if (s.status()) return 1;
  launch_attention32(prec, dq, dk, dv, dout, dl, S, H, Np, cross, s.stream());
  s.wait(HookStage::OWN_TEXT);
  const std::vector<uint16_t> ho = s.get<uint16_t>(dout, out_n + slack_n);
  const int rows_out = a->raw ? Np : n;
  for (int q = 0; q < S; ++q)
    for (int i = 0; i < rows_out; ++i)
      for (int f = 0; f < H * 64; ++f) a->out[((size_t)q * rows_out + i) * H * 64 + f] = back2(ho[((size_t)q * Np + i) * H * 64 + f], prec);
  for (int r = 0; r < 128 && a->canary; ++r) {
    bool changed = false;
    for (int f = 0; f < H * 64 && !changed; ++f) changed = ho[out_n + (size_t)r * H * 64 + f] != 0xFFFFu;
    a->rows_past += changed;
  }
  return s.status();
}

extern "C" {
int airfe_debug_attention(airfe_ctx* c, const float* q, const float* k, const float* v, const int* lens, int S, int H, int n, int cross, float* out) try {
  AIRFE_ENTER(c);
  if (c->mprec == 2) return fail(c, "debug_attention drives the 2-byte kernel (matcher_precision fp16 / bf16)");
  airfe_debug_attn_args a = {};
  a.prec = c->mprec; a.S = S; a.H = H; a.n = n; a.cross = cross;
  a.q = q; a.k = k; a.v = v; a.lens = lens; a.out = out;                 // canary = 0, raw = 0: a zero-filled output buffer, the first n rows back
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
  HookStage s(c, "debug_lg_prepare");
  const size_t fl = (size_t)B * a->cap * a->ld;
  std::vector<int> hn(2 * B + 2);
  for (int b = 0; b < B; ++b) { hn[b] = a->n0[b]; hn[B + b] = a->n1[b]; }
  hn[2 * B] = a->n0x; hn[2 * B + 1] = a->n1x;
  const int* dn = s.up(std::move(hn));
  LgPrepArgs pa;
  pa.f0 = s.up(a->f0, fl); pa.f1 = s.up(a->f1, fl); pa.wr = s.up(a->wr, (size_t)64);
  if (a->f0x) {
    std::vector<float> x0(a->f0x, a->f0x + (size_t)a->n0x * a->ld), x1(a->f1x, a->f1x + (size_t)a->n1x * a->ld);
    x0.resize(x0.size() + a->ld, 0.f); x1.resize(x1.size() + a->ld, 0.f);          // (never empty)
    pa.f0x = s.up(std::move(x0)); pa.f1x = s.up(std::move(x1));
  }
  const DevSpan arena[4] = {{c->x32, R * 256 * 4}, {c->xb, R * 256 * 2}, {c->rot_cos, R * 32 * 4}, {c->rot_sin, R * 32 * 4}};
  for (const DevSpan& e : arena) s.fill(e.p, 0xFF, e.bytes);
  s.fill(c->lens, 0xFF, (size_t)2 * c->Pmax * 4);
  if (s.status()) return 1;
  pa.n0 = dn; pa.n1 = dn + B; pa.ld = a->ld; pa.kp_off = a->kp_off; pa.normalize = a->normalize;
  pa.cx = a->cx; pa.cy = a->cy; pa.linv = a->linv; pa.B = B; pa.cap = a->cap; pa.Np = Np;
  pa.x32 = c->x32; pa.xb = c->xb; pa.rot_cos = c->rot_cos; pa.rot_sin = c->rot_sin; pa.lens = c->lens;
  if (a->f0x) { pa.n0x = dn + 2 * B; pa.n1x = dn + 2 * B + 1; }
  pa.slack_rows = a->slack_rows;
  launch_lg_prepare(a->prec, pa, s.stream());
  s.wait();
  const std::vector<float> hx = s.get<float>(c->x32, R * 256);
  const std::vector<uint16_t> hb = s.get<uint16_t>(c->xb, R * 256);
  s.get(a->rot_cos, c->rot_cos, rows * 32 * 4);
  s.get(a->rot_sin, c->rot_sin, rows * 32 * 4);
  s.get(a->lens, c->lens, (size_t)2 * Bt * 4);
  if (s.status()) return 1;
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
  for (const DevSpan& e : arena) s.fill(e.p, 0, e.bytes);
  return s.wait();
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
  HookStage s(c, "debug_lg_assign");
  const float* dw = s.up(a->w, (size_t)256);
  float* dscores = s.fresh<float>((size_t)B * blk, 0xFF);
  float* dscore = s.fresh<float>((size_t)B * cap, 0xFF);
  int* dnm = s.fresh<int>((size_t)B, 0xFF);
  int32_t* didx = s.fresh<int32_t>((size_t)B * cap * 2, 0);             // zero, not -1: the value that passes for a valid index
  s.put(c->mdb, std::move(hmd));
  s.put(c->x32, std::move(hx));
  s.put(c->lens, a->lens, (size_t)S * 4);
  const size_t bn = (size_t)B * Np * 4;
  const DevSpan nan_out[7] = {{c->zbuf, M * 4}, {c->simbuf, (size_t)B * blk * 4}, {c->lg_part, pf * 4}, {c->lg_argpart, pf * 4}, {c->rowlse, bn}, {c->collse, bn}, {c->rowval, bn}};
  for (const DevSpan& e : nan_out) s.fill(e.p, 0xFF, e.bytes);
  s.fill(c->rowarg, 0, bn);
  s.fill(c->colarg, 0, bn);
  if (s.status()) return 1;
  hipStream_t st = s.stream();
  launch_rowdot256(c->x32, dw, a->b, c->zbuf, (int)M, st);
  if (a->form == 1) {
    launch_lg_assign_fused(prec, c->mdb, c->zbuf, c->lens, B, Np, cap, a->thr, c->lg_part, c->lg_argpart, c->rowlse, c->collse, c->simbuf, dscores, c->rowarg,
                           c->rowval, c->colarg, didx, dscore, dnm, st);
  } else {
    launch_sim(prec, c->mdb, c->simbuf, B, Np, st);
    launch_lg_assign(c->simbuf, c->zbuf, c->lens, B, Np, cap, a->thr, c->rowlse, c->collse, dscores, c->rowarg, c->rowval, c->colarg, didx, dscore, dnm, st);
  }
  s.wait();
  const size_t nb = (size_t)n * 4, npb = (size_t)Np * 4;
  s.get2d(a->z, nb, c->zbuf, npb, nb, S);
  for (int b = 0; b < B; ++b) {
    s.get2d(a->sim + (size_t)b * n * n, nb, c->simbuf + b * blk, npb, nb, n);
    s.get2d(a->scores + (size_t)b * n * n, nb, dscores + b * blk, npb, nb, n);
  }
  const struct { void* h; const void* d; } rows[5] = {{a->rowlse, c->rowlse}, {a->collse, c->collse}, {a->rowval, c->rowval}, {a->rowarg, c->rowarg}, {a->colarg, c->colarg}};
  for (const auto& e : rows) s.get2d(e.h, nb, e.d, npb, nb, B);
  s.get(a->idx, didx, (size_t)B * cap * 8);
  s.get(a->score, dscore, (size_t)B * cap * 4);
  s.get(a->nmatch, dnm, (size_t)B * 4);
  s.fill(c->mdb, 0, M * 256 * 2);          // no NaN token rows stay behind
  s.fill(c->x32, 0, M * 256 * 4);
  s.fill(c->zbuf, 0, M * 4);
  return s.wait();
} AIRFE_CATCH(c)

/* ---- SuperGlue's front alone: sg_front_dev, the statement superglue_dev runs (include/airfe_debug.h; tests/test_gpu_sg_front.py) */
int airfe_debug_sg_front(airfe_ctx* c, airfe_debug_sg_front_args* a) try {
  AIRFE_ENTER(c);
  if (!c->has_sg) return fail(c, "debug_sg_front: SuperGlue not loaded");
  if (!a || !a->f0 || !a->f1 || !a->n0 || !a->n1 || !a->lens || !a->x32 || !a->xb || (a->split && (!a->h128 || !a->hb))) return fail(c, "debug_sg_front: null argument");
  const int Np = c->Np, B = a->B, cap = a->cap, prec = a->prec, split = a->split;
  if ((prec != 0 && prec != 1) || (split != 0 && split != 1) || B < 1 || B > c->Pmax || cap < 1 || cap > Np)
    return fail(c, "debug_sg_front: bad argument (prec 0 / 1, split 0 / 1, 1 <= B <= max_batch, 1 <= cap <= Np)");
  if (prec != (c->mprec == 2 ? 1 : c->mprec) || (split && c->mprec == 2))
    return fail(c, "debug_sg_front: prec must be the context's matcher_precision (fp32 context: 1, the shadow's type, and the unsplit form only)");
  for (int b = 0; b < B; ++b)
    if (a->n0[b] < 0 || a->n0[b] > cap || a->n1[b] < 0 || a->n1[b] > cap) return fail(c, "debug_sg_front: every n0, n1 must lie in 0 .. cap");
  const size_t M = (size_t)2 * B * Np, rows = (M + 127) / 128 * 128, R = c->arena_rows;
  if (rows > R || (size_t)a->rows != rows) return fail(c, "debug_sg_front: rows must be 2 B Np rounded up to 128 and fit the arena");
  HookStage s(c, "debug_sg_front");
  const size_t fl = (size_t)B * cap * AIRFE_FEAT_DIM;
  const float *d0 = s.up(a->f0, fl), *d1 = s.up(a->f1, fl);
  const int *dn0 = s.up(a->n0, (size_t)B), *dn1 = s.up(a->n1, (size_t)B);
  const DevSpan arena[5] = {{c->x32, R * 256 * 4}, {c->xb, R * 256 * 2}, {c->msg, R * 256 * 2}, {c->hb, R * 512 * 2}, {c->lens, (size_t)2 * c->Pmax * 4}};
  for (const DevSpan& e : arena) s.fill(e.p, 0xFF, e.bytes);
  if (s.status()) return 1;
  s.step(sg_front_dev(c, d0, dn0, d1, dn1, B, cap, a->normalize, split != 0, s.stream()));
  s.wait();
  const std::vector<float> hx = s.get<float>(c->x32, R * 256);
  const std::vector<uint16_t> hxb = s.get<uint16_t>(c->xb, R * 256), hh = s.get<uint16_t>(c->msg, split ? rows * 128 : 0), hhb = s.get<uint16_t>(c->hb, split ? rows * 256 : 0);
  s.get(a->lens, c->lens, (size_t)2 * B * 4);
  if (s.status()) return 1;
  memcpy(a->x32, hx.data(), rows * 256 * 4);
  dbg_back2(hxb, rows * 256, prec, a->xb);
  if (split) { dbg_back2(hh, rows * 128, prec, a->h128); dbg_back2(hhb, rows * 256, prec, a->hb); }
  int past = 0;
  for (size_t r = rows; r < R; ++r) {
    bool touched = false;
    for (int k = 0; k < 256 && !touched; ++k) {
      uint32_t u;
      memcpy(&u, &hx[r * 256 + k], 4);
      touched = (u != 0u && u != 0xFFFFFFFFu) || (hxb[r * 256 + k] != 0u && hxb[r * 256 + k] != 0xFFFFu);
    }
    past += touched;
  }
  a->rows_past = past;
  for (const DevSpan& e : arena) s.fill(e.p, 0, e.bytes);          // the arena as alloc_matcher_arena left it
  return s.wait();
} AIRFE_CATCH(c)

/* ---- the matchers' tails alone on HOST score matrices, staged into the arena */
/* filter_matches (src/light_glue.cpp:214-266) alone on one HOST score matrix [n0][n1] */
int airfe_debug_lg_filter(airfe_ctx* c, const float* scores, int n0, int n1, int32_t* idx, float* score, int cap, int* nmatch) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_arena) return fail(c, "debug_lg_filter: no matcher loaded");
  if (n0 < 1 || n1 < 1 || n0 > c->cfg.max_keypoints || n1 > c->cfg.max_keypoints || !scores || !idx || !score || !nmatch)
    return fail(c, "debug_lg_filter: bad argument");
  HookStage s(c, "debug_lg_filter");
  const int lens[2] = {n0, n1};
  s.put(c->lens, lens, 8);
  s.put2d(c->simbuf, (size_t)c->Np * 4, scores, (size_t)n1 * 4, (size_t)n1 * 4, n0);
  if (s.status()) return 1;
  launch_lg_filter_scores(c->simbuf, c->lens, 1, c->Np, c->Np, 0.1f, c->rowarg, c->rowval, c->colarg, c->st_idx, c->st_score, c->st_nm, s.stream());
  s.wait();
  int nm = 0;
  s.get(&nm, c->st_nm, 4);
  nm = std::min(nm, cap);
  s.get(idx, c->st_idx, (size_t)std::max(nm, 0) * 8);
  s.get(score, c->st_score, (size_t)std::max(nm, 0) * 4);
  *nmatch = nm;
  return s.status();
} AIRFE_CATCH(c)

/* decode (src/super_glue.cpp:339-367) alone on one HOST score matrix Z [n0+1][n1+1] */
int airfe_debug_sg_decode(airfe_ctx* c, const float* Z, int n0, int n1, int32_t* idx0, int32_t* idx1, double* ms0, double* ms1) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_sg) return fail(c, "debug_sg_decode: SuperGlue not loaded");
  if (n0 < 1 || n1 < 1 || n0 > c->cfg.max_keypoints || n1 > c->cfg.max_keypoints || !Z || !idx0 || !idx1 || !ms0 || !ms1)
    return fail(c, "debug_sg_decode: bad argument");
  HookStage s(c, "debug_sg_decode");
  const int lens[2] = {n0, n1};
  s.put(c->lens, lens, 8);
  s.put2d(c->sg_Z, (size_t)c->Lz * 4, Z, (size_t)(n1 + 1) * 4, (size_t)(n1 + 1) * 4, n0 + 1);
  if (s.status()) return 1;
  launch_sg_decode(c->sg_Z, c->lens, 1, c->Np, c->Lz, 0.2f, c->sg_idx0, c->sg_max0, c->sg_idx1, c->sg_out0, c->sg_out1, c->sg_ms0, c->sg_ms1, s.stream());
  s.wait();
  s.get(idx0, c->sg_out0, (size_t)n0 * 4);
  s.get(idx1, c->sg_out1, (size_t)n1 * 4);
  const std::vector<float> m0 = s.get<float>(c->sg_ms0, n0), m1 = s.get<float>(c->sg_ms1, n1);
  for (int i = 0; i < n0; ++i) ms0[i] = (double)m0[i];
  for (int j = 0; j < n1; ++j) ms1[j] = (double)m1[j];
  return s.status();
} AIRFE_CATCH(c)

/* launch_sg_sinkhorn alone on B HOST coupling matrices (include/airfe_debug.h).  Everything of the arena outside each pair's valid n0 x n1 block is NaN when
   the launch starts, and so is the output: a finite Z [0..n0][0..n1] was written in full and came from inside `lens` alone. */
int airfe_debug_sg_sinkhorn(airfe_ctx* c, const float* sim, const int* lens, int B, int ld, float alpha, int iters, int form, float* Z, int* form_ran) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_sg) return fail(c, "debug_sg_sinkhorn: SuperGlue not loaded");
  if (!sim || !lens || !Z || !form_ran || B < 1 || B > c->Pmax || ld < 1 || iters < 0 || form < 0 || form > 2)
    return fail(c, "debug_sg_sinkhorn: bad argument (1 <= B <= max_batch, iters >= 0, form 0 / 1 / 2)");
  const int nmax = std::min(ld, c->cfg.max_keypoints);
  for (int i = 0; i < 2 * B; ++i)
    if (lens[i] < 1 || lens[i] > nmax) return fail(c, "debug_sg_sinkhorn: every n0, n1 must lie in 1 .. min(ld, max_keypoints)");
  *form_ran = 0;
  const int Np = c->Np, Lz = c->Lz;
  const size_t blk = (size_t)Np * Np, zblk = (size_t)Lz * Lz;
  HookStage s(c, "debug_sg_sinkhorn");
  s.put(c->lens, lens, (size_t)B * 8);
  s.fill(c->simbuf, 0xFF, (size_t)B * blk * 4);          // 0xFFFFFFFF: a NaN
  s.fill(c->sg_Z, 0xFF, (size_t)B * zblk * 4);
  s.fill(c->sg_xch, 0xFF, (size_t)B * Lz * 64 * 4);      // [B][2][16][Lz] float2: a partial read before it was written is a NaN
  for (int b = 0; b < B; ++b)
    s.put2d(c->simbuf + b * blk, (size_t)Np * 4, sim + (size_t)b * ld * ld, (size_t)ld * 4, (size_t)lens[2 * b + 1] * 4, lens[2 * b]);
  if (s.status()) return 1;
  launch_sg_sinkhorn(c->simbuf, c->lens, B, Np, Lz, alpha, iters, c->sg_u, c->sg_v, c->sg_Z, c->sg_cnt, c->sg_cnt + (size_t)c->Pmax * 16, c->sg_xch, s.stream(),
                     form, form_ran);
  if (*form_ran == 0)
    return s.refuse("form 2 asked for, but no register-resident instantiation applies to this context (max_keypoints, B against the co-resident "
                    "workgroups) or the cooperative launch was refused");
  if (!s.wait()) s.step(sinkhorn_failed(c));
  for (int b = 0; b < B; ++b)
    s.get2d(Z + (size_t)b * (ld + 1) * (ld + 1), (size_t)(ld + 1) * 4, c->sg_Z + b * zblk, (size_t)Lz * 4, (size_t)(lens[2 * b + 1] + 1) * 4, lens[2 * b] + 1);
  return s.status();
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
  const size_t f0 = (size_t)B0 * cap * AIRFE_FEAT_DIM, f1 = (size_t)B1 * cap * AIRFE_FEAT_DIM;
  HookStage s(c, "debug_detector_tail");
  float* dfeat = s.up(a->feat, f0);
  int* dn = s.up(a->n, (size_t)B0);
  float* dfeat1 = two ? s.up(a->feat1, f1) : nullptr;
  int* dn1 = two ? s.up(a->n1, (size_t)B1) : nullptr;
  clear_saturation(c);
  s.put(c->heat, a->heat, px * 4);
  s.put(c->aDa, std::move(act));
  // detect_dev2's descriptor-head rule (point_desc_head), then its tail
  bool sparse_desc = false;
  if (!s.status()) s.step(point_desc_head(c, B, cap, s.stream(), sparse_desc));
  if (!s.status()) s.step(detect_tail_dev(c, B, Bs, two, sparse_desc, a->h, a->w, dfeat, dfeat1, cap, dn, dn1, s.stream()));
  s.wait(HookStage::SATURATION);
  s.get(a->feat, dfeat, f0 * 4);
  s.get(a->n, dn, (size_t)B0 * 4);
  if (two) {
    s.get(a->feat1, dfeat1, f1 * 4);
    s.get(a->n1, dn1, (size_t)B1 * 4);
  }
  a->nms_map_written = c->cfg.nms_radius > 0 && c->nms_map_valid;
  if (a->nms_map && a->nms_map_written) s.get(a->nms_map, c->heat_nms, px * 4);
  if (a->keep) s.get(a->keep, c->nms_mask, cells * 8);
  if (a->cand_cnt) s.get(a->cand_cnt, c->cand_cnt, (size_t)B * 4);
  return s.status();
} AIRFE_CATCH(c)

}  // extern "C"

// what line_post and junction_tail share.  In: stage 1's lines_adjusted | scores rows and kept counts m2, the point branch's score map, the caller's line / junction rows and
// the four count rows nlines | nfound | njunc | jfound as 0xFF.  Out: the same rows and counts.
struct DbgLineIo { double* lines = nullptr; float* junc = nullptr; int* cnt = nullptr; };
template <class A>
static DbgLineIo dbg_line_stage(HookStage& s, airfe_ctx* c, const A* a) {
  const int B = a->B, nj = a->nj, ld = a->ld, R = AIRFE_INTERNAL_SIZE;
  DbgLineIo io;
  io.lines = s.up(a->lines, (size_t)B * a->capL * 4);
  if (nj > 0) io.junc = s.up(a->junc, (size_t)nj * a->capJ * AIRFE_FEAT_DIM);
  io.cnt = s.fresh<int>((size_t)4 * B, 0xFF);
  clear_saturation(c);
  std::vector<int> counts((size_t)B * LINE_CNT_LD, 0);
  for (int b = 0; b < B; ++b) counts[(size_t)b * LINE_CNT_LD + 1] = a->m2[b];
  s.put2d(c->s1_la, (size_t)LINE_CAP * 16, a->la, (size_t)ld * 16, (size_t)ld * 16, B);
  s.put2d(c->s1_sc, (size_t)LINE_CAP * 4, a->sc, (size_t)ld * 4, (size_t)ld * 4, B);
  s.put(c->wf_counts, std::move(counts));
  c->wf_counted = false;                                     // (the per-workgroup counts of a previous line branch are gone)
  s.put(c->heat, a->heat, (size_t)B * R * R * 4);
  return io;
}
template <class A>
static int dbg_line_back(HookStage& s, A* a, const DbgLineIo& io) {
  const size_t B = a->B, nj = a->nj;
  s.get(a->lines, io.lines, B * a->capL * 32);
  s.get(a->nlines, io.cnt, B * 4);
  s.get(a->nfound, io.cnt + B, B * 4);
  if (nj > 0) {
    s.get(a->junc, io.junc, nj * a->capJ * AIRFE_FEAT_DIM * 4);
    s.get(a->njunc, io.cnt + 2 * B, nj * 4);
    s.get(a->jfound, io.cnt + 3 * B, nj * 4);
  }
  return s.status();
}

extern "C" {

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
  HookStage s(c, "debug_line_post");
  const DbgLineIo io = dbg_line_stage(s, c, a);
  if (s.status()) return 1;
  hipStream_t st = s.stream();
  // the point branch's NMS as detect_tail_dev runs it: with the dense map (one- and two-image calls) or with the keep plane alone (larger batches)
  c->nms_map_valid = !a->from_plane;
  launch_nms512_candidates(c->heat, c->nms_map_valid ? c->heat_nms : nullptr, c->nms_mask, B, c->cfg.keypoint_threshold, c->cfg.remove_borders, c->cand, c->cand_cnt,
                           R * R, st);
  // line_post_dev's steps without the descriptor sampling (line_filter_maps, junction_scan_maps), images 0 .. B-1, junctions of the first nj
  junction_maps_clear(c, nj, st);
  line_filter_maps(c, B, nj, a->h, a->w, io.lines, capL, io.cnt, io.cnt + B, st);
  // a caller's junction maps instead of the filter's, between the two launches: the scan's own bounds (the filter never marks a pixel the scan would reject)
  if (nj > 0 && a->jmap) s.put(c->jmap, a->jmap, (size_t)nj * R * R);
  if (nj > 0 && !s.status()) s.step(junction_scan_maps(c, 0, nj, io.junc, capJ, io.cnt + 2 * B, io.cnt + 3 * B, st));
  s.wait(HookStage::SATURATION);
  return dbg_line_back(s, a, io);
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
  HookStage s(c, "debug_junction_tail");
  const DbgLineIo io = dbg_line_stage(s, c, a);
  s.put(c->aDa, std::move(act));
  if (s.status()) return 1;
  hipStream_t st = s.stream();
  // the point branch as detect_dev2 / detect_tail_dev leave it: one- and two-image calls keep the dense NMS'd map and the dense descriptor map, larger batches the keep
  // plane alone (their descriptor head ran over the sampled cells)
  c->nms_map_valid = B <= 2;
  launch_nms512_candidates(c->heat, c->nms_map_valid ? c->heat_nms : nullptr, c->nms_mask, B, c->cfg.keypoint_threshold, c->cfg.remove_borders, c->cand, c->cand_cnt,
                           R * R, st);
  c->desc_dense_valid = false;
  c->last_B = B;
  if (B <= 2) {
    s.step(dense_desc_head(c, B, st));
    c->desc_dense_valid = true;
  }
  // plnet_lines_batch's rule (junction_dense_maps), then line_tail_dev's clear of the byte maps and its end
  bool partial = false;
  if (!s.status()) s.step(junction_dense_maps(c, nj, capJ, 3, st, partial));
  const bool fused = junction_tail_fused(c, nj, capJ);
  if (!s.status() && !fused) junction_maps_clear(c, nj, st);
  if (!s.status()) s.step(line_post_dev(c, 0, B, a->h, a->w, io.lines, capL, io.cnt, io.cnt + B, io.junc, capJ, io.cnt + 2 * B, io.cnt + 3 * B, nj, st, 3, fused));
  if (partial) c->desc_dense_valid = false;
  if (s.wait(HookStage::SATURATION)) return 1;
  a->fused = fused ? 1 : 0;
  return dbg_line_back(s, a, io);
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
  HookStage s(c, "debug_line_mid");
  float* d = c->s0_stage;
  clear_saturation(c);
  // ---- staging: the stage block (juncs | lines_pred | iskeep | min | max | thin | aux), the pixel-major thin | aux copy; 0xFF everywhere the device writes
  std::vector<float> ta8((size_t)B * NPX * 8);
  for (int b = 0; b < B; ++b)
    for (int ch = 0; ch < 8; ++ch) {
      const float* src = (ch < 4 ? a->thin : a->aux) + ((size_t)b * 4 + (ch & 3)) * NPX;
      for (int p = 0; p < NPX; ++p) ta8[((size_t)b * NPX + p) * 8 + ch] = src[p];
    }
  s.put(c->l_ta8, std::move(ta8));
  const size_t blk = SG_STRIDE * 4, np4 = (size_t)NP * 4, pl4 = (size_t)4 * NPX * 4;      // one image's stage block, a kept-proposal row, four planes: in bytes
  s.put2d(d + SG_JUNCS, blk, a->juncs_pred, 600 * 4, 600 * 4, B);
  s.put2d(d + SG_LP, blk, a->lines_pred, np4 * 4, np4 * 4, B);
  s.put2d(d + SG_THIN, blk, a->thin, pl4, pl4, B);
  s.put2d(d + SG_AUX, blk, a->aux, pl4, pl4, B);
  static_assert(SG_MIN == SG_KEEP + KEEP_CAP && SG_MAX == SG_MIN + KEEP_CAP, "iskeep | min | max are contiguous");
  if (a->j2l == 0) {
    s.put2d(d + SG_KEEP, blk, a->iskeep_in, np4, np4, B);
    s.put2d(d + SG_MIN, blk, a->idx_min_in, np4, np4, B);
    s.put2d(d + SG_MAX, blk, a->idx_max_in, np4, np4, B);
  } else {
    for (int b = 0; b < B; ++b) s.fill(d + (size_t)b * SG_STRIDE + SG_KEEP, 0xFF, 3 * np4);          // (iskeep | min | max are one run of the block)
  }
  const size_t L = (size_t)B;
  const DevSpan outs[9] = {{c->wf_counts, L * LINE_CNT_LD * 4}, {c->wf_keep, L * KEEP_CAP * 4}, {c->wf_pairs, L * LINE_CAP * 8}, {c->wf_rep, L * LINE_CAP * 4},
                           {c->wf_prop, L * LINE_CAP * 16}, {c->s1_la, L * LINE_CAP * 16}, {c->s1_sc, L * LINE_CAP * 4}, {c->s1_jfeat, L * 300 * 256 * 4},
                           {c->l_ridx, L * 1200 * 4}};
  for (const DevSpan& e : outs) s.fill(e.p, 0xFF, e.bytes);
  if (s.status()) return 1;
  hipStream_t st = s.stream();
  // ---- line_branch_dev's match (line_match)
  c->wf_counted = false;                                     // (j2l = 0: the caller's match, which nothing has counted)
  if (a->j2l) line_match(c, B, a->j2l == 1, st);
  if (a->j2l == 2 && !c->wf_counted) return s.refuse("the cell search did not leave the per-workgroup counts (the line path's form)");
  // ---- line_tail_dev: the kept list and the unique pairs (line_dedup)
  line_dedup(c, B, st);
  s.wait();
  s.get(a->head4, c->s1_la, L * LINE_CAP * 16);
  if (form != 3) s.fill(c->s1_la, 0xFF, L * LINE_CAP * 16);      // stage 1 of forms 0 .. 2 writes lines_adjusted itself
  // ---- the junction projections and stage 1
  if (form == 0) {
    std::vector<float> chw((size_t)128 * NPX);
    for (int p = 0; p < NPX; ++p)
      for (int ch = 0; ch < 128; ++ch) chw[(size_t)ch * NPX + p] = a->loi[(size_t)p * 128 + ch];
    s.put(c->s0_loi, std::move(chw));
  } else if (form == 1) {
    std::vector<float> head((size_t)NPX * 160);
    memset(head.data(), 0xFF, head.size() * 4);              // (columns 128 .. 159: the 17 decoded channels, which nothing behind stage 0 reads)
    for (int p = 0; p < NPX; ++p) memcpy(&head[(size_t)p * 160], a->loi + (size_t)p * 128, 128 * 4);
    s.put(c->l_head, std::move(head));
  } else {
    const int M = B * 1200;
    if (!s.status()) s.step(line_tap_rows(c, B, s.stream()));
    s.wait();
    const std::vector<int> ridx = s.get<int>(c->l_ridx, (size_t)M);
    if (s.status()) return 1;
    std::vector<float> lrows((size_t)M * 128);
    for (int r = 0; r < M; ++r) {                            // what the gather GEMM (line_loi_rows) hands on: row ridx[r] of the [B * 128*128][128] line-feature matrix
      const int b = r / 1200;
      if (ridx[r] < b * NPX || ridx[r] >= (b + 1) * NPX) return s.refuse("launch_s1_junc_rows listed a row outside its image");
      memcpy(&lrows[(size_t)r * 128], a->loi + (size_t)ridx[r] * 128, 128 * 4);
    }
    s.put(c->l_lrows, std::move(lrows));
  }
  static_assert(S1_CHW == 0 && S1_HEAD == 1 && S1_ROWS == 2 && S1_ROWS_H == 3, "s1_form (include/airfe_debug.h) is S1Form's first four");
  if (s.status()) return 1;
  line_stage1(c, B, form, a->wgs, s.stream());
  s.wait(HookStage::SATURATION);
  // ---- everything back as the device left it
  s.get2d(a->iskeep, np4, d + SG_KEEP, blk, np4, B);
  s.get2d(a->idx_min, np4, d + SG_MIN, blk, np4, B);
  s.get2d(a->idx_max, np4, d + SG_MAX, blk, np4, B);
  s.get2d(a->counts, 8, c->wf_counts, LINE_CNT_LD * 4, 8, B);
  s.get(a->keep, c->wf_keep, L * KEEP_CAP * 4);
  s.get(a->pairs, c->wf_pairs, L * LINE_CAP * 8);
  s.get(a->rep, c->wf_rep, L * LINE_CAP * 4);
  s.get(a->prop4, c->wf_prop, L * LINE_CAP * 16);
  if (form >= 2) s.get(a->ridx, c->l_ridx, L * 1200 * 4);
  if (form >= 1) s.get(a->proj, c->s1_jfeat, L * 300 * 256 * 4);
  s.get(a->lines_adjusted, c->s1_la, L * LINE_CAP * 16);
  s.get(a->scores_line, c->s1_sc, L * LINE_CAP * 4);
  const std::vector<int> table = s.get<int>(c->wf_table, L * 300 * 300);
  for (int b = 0; b < B; ++b) {
    int dirty = 0;
    for (size_t i = 0; i < (size_t)300 * 300; ++i) dirty += table[(size_t)b * 300 * 300 + i] != 0x7FFFFFFF;
    a->table_dirty[b] = dirty;
  }
  return s.status();
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
  float* d = c->s0_stage;
  clear_saturation(c);
  HookStage s(c, "debug_s0_decode", mode ? a->prec : 0);
  float* djnms = s.fresh<float>((size_t)B * NPX, 0xFF);
  float* jnms = a->want_jnms ? djnms : nullptr;
  // ---- every output 0xFF
  const DevSpan outs[6] = {{d, (size_t)B * SG_STRIDE * 4}, {c->l_jloc, (size_t)B * NPX * 4}, {c->l_joff, (size_t)B * 2 * NPX * 4}, {c->l_ta8, (size_t)B * 8 * NPX * 4},
                           {c->s0_loi, (size_t)128 * NPX * 4}, {c->l_dec, mode == 2 ? (size_t)B * NPX * 32 * 4 : 0}};
  for (const DevSpan& e : outs) s.fill(e.p, 0xFF, e.bytes);
  if (mode == 0) {
    const size_t n = (size_t)B * NPX * a->ld;
    float* head = a->ld == 32 ? c->l_dec : c->l_head;
    if (a->ld == 160 && B > 1) head = s.up(a->rows, n);      // (l_head holds one image)
    else s.put(head, a->rows, n * 4);
    if (s.status()) return 1;
    line_decode_rows(c, B, head, a->ld, a->off, jnms, a->want_ta8 != 0, a->want_loi != 0, s.stream());
  } else {
    const size_t n = (size_t)B * NPX * 128;
    std::vector<uint16_t> xin(n);
    for (size_t i = 0; i < n; ++i) xin[i] = cvt2(a->x[i], a->prec);
    LinW lw;
    s.linear(a->w, a->b, 128, 17, lw);
    s.put(c->l_feat, std::move(xin));
    if (s.status()) return 1;
    if (mode == 1) {
      line_head_decode(c, B, a->prec, lw, jnms, a->wgs, s.stream());
    } else {                                                 // (fuse_dec = 0: the 17-channel head as a GEMM, then the decode over its rows)
      line_head_gemm(c, B, false, a->prec, lw, s.stream());
      line_decode_rows(c, B, c->l_dec, 32, 0, jnms, true, false, s.stream());
    }
  }
  s.wait(HookStage::SATURATION);
  // ---- everything back as the device left it
  s.get(a->stage, d, (size_t)B * SG_STRIDE * 4);
  s.get(a->jloc, c->l_jloc, (size_t)B * NPX * 4);
  s.get(a->joff, c->l_joff, (size_t)B * 2 * NPX * 4);
  s.get(a->jnms, djnms, (size_t)B * NPX * 4);
  s.get(a->ta8, c->l_ta8, (size_t)B * 8 * NPX * 4);
  s.get(a->loi, c->s0_loi, (size_t)128 * NPX * 4);
  if (mode == 2) s.get(a->head_rows, c->l_dec, (size_t)B * NPX * 32 * 4);
  if (!s.status()) c->wf_counted = false;                    // (the stage blocks no longer hold a line branch's match)
  return s.status();
} AIRFE_CATCH(c)

int airfe_debug_junctions_topk(airfe_ctx* c, const float* jloc, const float* joff, int B, float* juncs_pred) try {
  AIRFE_ENTER(c);
  if (!c->has_s0 || !c->s0_stage) return fail(c, "debug_junctions_topk: the line branch is not loaded (line.* tensors, cfg.plnet_s1_pack)");
  if (!jloc || !joff || !juncs_pred || B < 1 || B > c->Lmax) return fail(c, "debug_junctions_topk: bad argument (1 <= B <= the arena's images)");
  const size_t npx = 128 * 128;
  HookStage s(c, "debug_junctions_topk");
  clear_saturation(c);
  s.put(c->l_jloc, jloc, (size_t)B * npx * 4);
  s.put(c->l_joff, joff, (size_t)B * 2 * npx * 4);
  if (s.status()) return 1;
  junctions_topk_dev(c, B, s.stream());
  s.wait(HookStage::SATURATION);
  s.get2d(juncs_pred, 600 * 4, c->s0_stage + SG_JUNCS, SG_STRIDE * 4, 600 * 4, B);
  return s.status();
} AIRFE_CATCH(c)

int airfe_debug_detector_maps(airfe_ctx* c, int B, float* heat_raw, float* heat_nms, float* desc) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_sp || B > c->Dmax) return 1;
  HookStage s(c, "debug_detector_maps");
  const size_t R = AIRFE_INTERNAL_SIZE;
  if (s.wait()) return 1;
  if (heat_raw) s.get(heat_raw, c->heat, (size_t)B * R * R * 4);
  if (heat_nms && c->cfg.nms_radius > 0 && !c->nms_map_valid) {      // the batch path skipped the dense map: rebuild it from the heat maps
    launch_nms512_candidates(c->heat, c->heat_nms, c->nms_mask, (int)B, c->cfg.keypoint_threshold, c->cfg.remove_borders, c->cand, c->cand_cnt,
                             R * R, s.stream());         // (the map is only ever skipped on the radius-4 path)
    if (s.wait()) return 1;
    c->nms_map_valid = true;
  }
  if (heat_nms) s.get(heat_nms, c->cfg.nms_radius > 0 ? c->heat_nms : c->heat, (size_t)B * R * R * 4);
  if (desc) {
    if (!c->desc_dense_valid) {     // the batch path ran the head on the sampled cells only: build the dense map from the kept activations
      s.step(dense_desc_head(c, c->last_B, s.stream()));
      c->desc_dense_valid = true;
    }
    if (!c->desc_normalised && !s.status()) {      // the inspection hook returns the map the reference would hold: normalised
      launch_l2norm256(c->desc, c->Dmax * 64 * 64, s.stream());
      if (s.wait()) return 1;
      c->desc_normalised = true;
    }
    s.get(desc, c->desc, (size_t)B * 64 * 64 * 256 * 4);
  }
  return s.status();
} AIRFE_CATCH(c)

/* the on-device stage-0 line branch of the LAST detected image, copied out in the Appendix A.1 layouts (NULL = skip) */
int airfe_debug_plnet_stage0(airfe_ctx* c, float* juncs_pred, float* lines_pred, float* iskeep, float* idx_min, float* idx_max,
                             float* loi, float* thin, float* aux, float* jloc, float* joff) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_s0 || !c->has_s1) return fail(c, "debug_plnet_stage0: line branch / stage 1 not loaded");
  HookStage s(c, "debug_plnet_stage0");
  s.step(line_branch_dev(c, s.stream(), 0, 1, true));
  s.wait();
  const size_t NP = KEEP_CAP;
  float* d = c->s0_stage;
  struct { float* h; const float* dv; size_t n; } cp[10] = {
      {juncs_pred, d + SG_JUNCS, 600}, {lines_pred, d + SG_LP, NP * 4}, {iskeep, d + SG_KEEP, NP}, {idx_min, d + SG_MIN, NP},
      {idx_max, d + SG_MAX, NP}, {loi, c->s0_loi, (size_t)128 * 128 * 128}, {thin, d + SG_THIN, (size_t)4 * 128 * 128},
      {aux, d + SG_AUX, (size_t)4 * 128 * 128}, {jloc, c->l_jloc, (size_t)128 * 128}, {joff, c->l_joff, (size_t)2 * 128 * 128}};
  for (auto& e : cp)
    if (e.h) s.get(e.h, e.dv, e.n * 4);
  return s.status();
} AIRFE_CATCH(c)

/* the junction-to-line match of the LAST detected image as the line path runs it (fast = 1: cell search, exact where it is consumed) or
   as the inspection hook exports it (fast = 0: every proposal against every junction): iskeep, idx_junc_to_end_min / _max [3*128*128] */
int airfe_debug_plnet_j2l(airfe_ctx* c, int fast, float* iskeep, float* idx_min, float* idx_max) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_s0 || !c->has_s1) return fail(c, "debug_plnet_j2l: line branch / stage 1 not loaded");
  HookStage s(c, "debug_plnet_j2l");
  s.step(line_branch_dev(c, s.stream(), 0, 1, fast == 0));
  s.wait();
  const size_t NP = KEEP_CAP;
  float* d = c->s0_stage;
  if (iskeep) s.get(iskeep, d + SG_KEEP, NP * 4);
  if (idx_min) s.get(idx_min, d + SG_MIN, NP * 4);
  if (idx_max) s.get(idx_max, d + SG_MAX, NP * 4);
  return s.status();
} AIRFE_CATCH(c)

// stage 1's kept count, then that many lines_adjusted [k][4] + scores_line [k] rows (at most cap), after the hook's wait
static int dbg_s1_rows(HookStage& s, airfe_ctx* c, float* lines_adjusted, float* scores_line, int cap, int* m2) {
  int cnt[2] = {0, 0};
  s.get(cnt, c->wf_counts, 8);
  const int k = std::max(std::min(cnt[1], cap), 0);
  s.get(lines_adjusted, c->s1_la, (size_t)k * 16);
  s.get(scores_line, c->s1_sc, (size_t)k * 4);
  if (!s.status()) *m2 = std::min(cnt[1], cap);
  return s.status();
}

/* stage-1 alone on HOST stage-0 tensors: lines_adjusted [M2][4] + scores_line [M2] (parity vs the real plnet_s1.onnx) */
int airfe_debug_plnet_s1(airfe_ctx* c, const airfe_plnet_stage0* s0, float* lines_adjusted, float* scores_line, int cap, int* m2) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_s1 || !s0) return fail(c, "debug_plnet_s1: stage-1 not loaded");
  HookStage s(c, "debug_plnet_s1");
  s.step(upload_stage0(c, s0, s.stream()));
  if (s.status()) return 1;
  line_dedup(c, 1, s.stream());                // (upload_stage0 left wf_counted false: host tensors, nothing has counted their kept proposals)
  line_stage1(c, 1, S1_CHW, 0, s.stream());
  s.wait();
  return dbg_s1_rows(s, c, lines_adjusted, scores_line, cap, m2);
} AIRFE_CATCH(c)

int airfe_debug_plnet_s1_last(airfe_ctx* c, float* lines_adjusted, float* scores_line, int cap, int* m2) try {
  if (c && enter_device(c)) return 1;
  if (!c || !c->has_s1 || !lines_adjusted || !scores_line || !m2) return fail(c, "debug_plnet_s1_last: stage-1 not loaded / bad argument");
  HookStage s(c, "debug_plnet_s1_last");
  s.wait(HookStage::DEVICE_WIDE);              // the last entry may have run the line path on the second stream
  return dbg_s1_rows(s, c, lines_adjusted, scores_line, cap, m2);
} AIRFE_CATCH(c)

/* csrc/wg_prims.h alone on HOST arrays, in one workgroup */
int airfe_debug_wg_prims(airfe_ctx* c, airfe_debug_wg_prims_args* a) try {
  if (c && enter_device(c)) return 1;
  if (!c || !a) return fail(c, "debug_wg_prims: bad argument");
  const bool sizes = (a->threads == 64 || a->threads == 256 || a->threads == 1024) && a->n >= 0 && a->n <= (1 << 20) && (a->key_bytes == 4 || a->key_bytes == 8) &&
                     a->P >= 0 && (a->P & (a->P - 1)) == 0 && (size_t)a->P * a->key_bytes <= 32768;
  if (!sizes || !a->totals || !a->wave || (a->n && (!a->v || !a->keep || !a->scan || !a->pos)) || (a->P && (!a->keys || !a->sorted)))
    return fail(c, "debug_wg_prims: bad argument");
  HookStage s(c, "debug_wg_prims");
  const size_t n = a->n, kb = (size_t)a->P * a->key_bytes, n_out = 2 * n + 5 + 3 * (a->threads / 64);
  const int* v = s.up(a->v, n);
  const uint8_t* keep = s.up(a->keep, n);
  const uint8_t* keys = s.up(static_cast<const uint8_t*>(a->keys), kb);
  int* out = s.fresh<int>(n_out, 0xFF);                           // scan | pos | totals | wave
  uint8_t* sorted = s.fresh<uint8_t>(kb, 0xFF);
  if (s.status()) return 1;
  if (a->threads == 64) launch_wg_prims<64>(a, v, keep, keys, out, sorted, s.stream());
  else if (a->threads == 256) launch_wg_prims<256>(a, v, keep, keys, out, sorted, s.stream());
  else launch_wg_prims<1024>(a, v, keep, keys, out, sorted, s.stream());
  s.wait(HookStage::OWN_TEXT);
  s.get(a->scan, out, n * 4);
  s.get(a->pos, out + n, n * 4);
  s.get(a->totals, out + 2 * n, 5 * 4);
  s.get(a->wave, out + 2 * n + 5, (size_t)3 * (a->threads / 64) * 4);
  s.get(a->sorted, sorted, kb);
  return s.status();
} AIRFE_CATCH(c)

}  // extern "C"
