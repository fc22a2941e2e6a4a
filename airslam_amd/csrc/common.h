// airfe — shared device/host helpers for the gfx950 front-end kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>

namespace airfe {

// Function attributes (hipFuncSetAttribute) and occupancy answers are per DEVICE, not per process: launchers keep one of these per kernel
// instantiation instead of a `static bool` (two contexts on two devices in one process — cfg.device invites it — would have left the second
// device's kernels without their dynamic-LDS limit).
struct PerDeviceOnce {
  // Thread-safe (round 6): two host threads driving two contexts may reach a kernel's FIRST launch together.  The one that gets here first runs the caller's
  // `if (auto once = x.first()) { hipFuncSetAttribute(...) }` body while holding the lock (the token lives as long as the if statement); the other waits for it and then
  // sees `done` — it can no longer launch a kernel whose dynamic-LDS limit is still being raised.  Behind the first use the fast path is one acquire load.
  std::atomic<bool> done[64] = {};
  std::mutex mu;
  struct Token {
    PerDeviceOnce* owner = nullptr;
    int dev = 0;
    bool yes = false;
    std::unique_lock<std::mutex> lock;
    Token() = default;
    Token(Token&& o) noexcept : owner(o.owner), dev(o.dev), yes(o.yes), lock(std::move(o.lock)) { o.owner = nullptr; }
    Token(const Token&) = delete;
    Token& operator=(const Token&) = delete;
    explicit operator bool() const { return yes; }
    ~Token() { if (owner) owner->done[dev].store(true, std::memory_order_release); }      // (before the lock member lets go)
  };
  Token first() {
    Token t;
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) { t.yes = true; return t; }      // (unknown device: set the attribute every time)
    if (done[d].load(std::memory_order_acquire)) return t;
    std::unique_lock<std::mutex> lk(mu);
    if (done[d].load(std::memory_order_relaxed)) return t;
    t.owner = this; t.dev = d; t.yes = true; t.lock = std::move(lk);
    return t;
  }
};


// `std::exp(float)` as the reference's host code computes it, for the two places where an exponential becomes an OUTPUT or meets a THRESHOLD (filter_matches
// src/light_glue.cpp:248-249, decode src/super_glue.cpp:299,355).  OCML's expf is a 1-ulp routine: beside the compiled reference (oracle/_ref,
// tests/test_gpu_ref_pin.py) it differed in the last bit of 7 % of the match scores.  Rounds 3-4 used (float)exp((double)x) — the correctly rounded value — which
// is what glibc returns "in practice" but not always: its expf has 0.502 ulp, and against the host's libm the correctly rounded value differs on 0.063 % of the
// inputs (37902 of 6e7 sampled), i.e. on one of ~200 match scores in every eighth pair (round 5: it turned tests/test_gpu_ref_pin.py red the moment the scores
// moved).  So this IS glibc's algorithm (glibc >= 2.27, sysdeps/ieee754/flt-32/e_expf.c with the exp2f_data table: x N / ln 2 = k + r by the 1.5 * 2^52 shift,
// 2^(k / N) from a 32-entry table, a cubic in r, all in double) with the contractions of the FMA build x86-64 hosts select (__expf_fma: r = fma(InvLn2N, x, -k),
// the only one of its fused operations that is visible in the results).  Verified on the CPU against glibc 2.35's expf on EVERY float (2 x 2139095041 values, 0
// mismatches: tools/expf_glibc_check.c); double arithmetic on the device is IEEE, so the bits carry over.  The call sites see at most 1024 values per pair.
__device__ __forceinline__ float expf_like_glibc(float x) {
  constexpr unsigned long long T[32] = {
      0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull,
      0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull, 0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull,
      0x3feeab07dd485429ull, 0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull, 0x3feeace5422aa0dbull,
      0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull, 0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
      0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
  constexpr double InvLn2N = 0x1.71547652b82fep+0 * 32, SHIFT = 0x1.8p+52;
  constexpr double C0 = 0x1.c6af84b912394p-5 / 32 / 32 / 32, C1 = 0x1.ebfce50fac4f3p-3 / 32 / 32, C2 = 0x1.62e42ff0c52d6p-1 / 32;
  if (x != x) return x + x;
  if (x > 0x1.62e42ep6f) return __builtin_inff();                    // overflow
  if (x < -0x1.9fe368p6f) return 0.0f;                               // below the smallest subnormal (also -inf)
  const double xd = (double)x;
  double kd = __builtin_fma(InvLn2N, xd, SHIFT);
  const unsigned long long ki = __builtin_bit_cast(unsigned long long, kd);
  kd -= SHIFT;
  const double r = __builtin_fma(InvLn2N, xd, -kd);
  const double s = __builtin_bit_cast(double, T[ki % 32] + (ki << 47));
  const double z = __builtin_fma(C0, r, C1);
  const double r2 = r * r;
  double y = __builtin_fma(C2, r, 1.0);
  y = __builtin_fma(z, r2, y);
  const double ys = y * s;
  return (float)ys;
}


typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(2))) short s16x2;

// ---------------------------------------------------------------------------------------------
// Precision traits: 2-byte storage type + the 16x16x32 MFMA that consumes it (fp32 accumulate).
// Storage in HBM/LDS is always raw uint16_t bits; these only give meaning to the bits.
struct PBF16 {
  using vec8 = bf16x8;
  static __device__ __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint16_t from_f32(float f) {
    __bf16 h = static_cast<__bf16>(f);
    return __builtin_bit_cast(uint16_t, h);
  }
  static __device__ __forceinline__ uint32_t pack2(float a, float b) {   // one v_cvt_pk_bf16_f32 (round to nearest even)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
  }
  static __device__ __forceinline__ float to_f32(uint16_t u) {
    return __builtin_bit_cast(float, (uint32_t)u << 16);
  }
};
struct PF16 {
  using vec8 = f16x8;
  static __device__ __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint16_t from_f32(float f) {
    _Float16 h = static_cast<_Float16>(f);
    return __builtin_bit_cast(uint16_t, h);
  }
  static __device__ __forceinline__ uint32_t pack2(float a, float b) {   // one v_cvt_pk_f16_f32 (round to nearest even)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, f16x2));
  }
  static __device__ __forceinline__ float to_f32(uint16_t u) {
    return static_cast<float>(__builtin_bit_cast(_Float16, u));
  }
};

template <class P>
__device__ __forceinline__ uint4 pack8(const float* v) {
  uint4 r;
  r.x = P::pack2(v[0], v[1]);
  r.y = P::pack2(v[2], v[3]);
  r.z = P::pack2(v[4], v[5]);
  r.w = P::pack2(v[6], v[7]);
  return r;
}
// ReLU on packed 2-byte floats (bf16 and fp16 alike): as signed 16-bit integers every negative float is negative, so
// one v_pk_max_i16 against 0 per PAIR replaces two fp32 max (+ canonicalisation) per value; -0 becomes +0.
__device__ __forceinline__ uint32_t relu_packed(uint32_t u) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, u), s16x2{0, 0}));
}
// max of packed 2-byte floats through v_pk_max_i16.  Exact whenever a ReLU follows: a non-negative float beats any negative
// one, two non-negative ones order like integers, and two negative ones give "some negative value" that the ReLU zeroes.
__device__ __forceinline__ uint32_t max_packed_pre_relu(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ uint4 max_packed_pre_relu(uint4 a, uint4 b) {
  return uint4{max_packed_pre_relu(a.x, b.x), max_packed_pre_relu(a.y, b.y), max_packed_pre_relu(a.z, b.z), max_packed_pre_relu(a.w, b.w)};
}
// value held by the horizontally adjacent lane (lane ^ 1): one DPP move (quad_perm [1,0,3,2]), no LDS crossbar trip
__device__ __forceinline__ uint32_t dpp_xor1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ uint4 dpp_xor1(uint4 v) { return uint4{dpp_xor1(v.x), dpp_xor1(v.y), dpp_xor1(v.z), dpp_xor1(v.w)}; }
__device__ __forceinline__ uint4 relu_packed(uint4 u) {
  return uint4{relu_packed(u.x), relu_packed(u.y), relu_packed(u.z), relu_packed(u.w)};
}
template <class P>
__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d) {
  uint2 r;
  r.x = P::pack2(a, b);
  r.y = P::pack2(c, d);
  return r;
}
template <class P>
__device__ __forceinline__ void unpack8(uint4 u, float* v) {
  v[0] = P::to_f32(u.x & 0xFFFF); v[1] = P::to_f32(u.x >> 16);
  v[2] = P::to_f32(u.y & 0xFFFF); v[3] = P::to_f32(u.y >> 16);
  v[4] = P::to_f32(u.z & 0xFFFF); v[5] = P::to_f32(u.z >> 16);
  v[6] = P::to_f32(u.w & 0xFFFF); v[7] = P::to_f32(u.w >> 16);
}

// ---------------------------------------------------------------------------------------------
// LDS swizzles (16-byte chunk index XOR) that keep ds_read_b128 MFMA-fragment reads conflict-free.
//   row pitch 128 B (64 two-byte channels): two rows share one 256-B bank row
//   row pitch >= 256 B                    : each row starts a bank row
__device__ __forceinline__ int swz128(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int swz256(int row) { return row & 15; }

// Weight slab: [64 rows][64 k] two-byte elements = 8 KiB, pitch 128 B, swz128.  Slab row (t,i)
// (MFMA tile t = 0..3, fragment row i = 0..15) holds output feature
//     co = (t>>1)*32 + (i>>2)*8 + (t&1)*4 + (i&3)
// so that after the swapped-operand MFMA (A = weights, B = activations) lane (j, g = lane>>4)
// owns features tp*32 + g*8 .. +8 of token/pixel j for tp = 0,1  ->  two 16-byte stores.
constexpr int SLAB_BYTES = 8192;

__host__ __device__ inline int slab_row_to_feature(int rr) {
  int t = rr >> 4, i = rr & 15;
  return (t >> 1) * 32 + (i >> 2) * 8 + (t & 1) * 4 + (i & 3);
}

template <class P>
__device__ __forceinline__ typename P::vec8 lds_frag(const char* base, int byte_off) {
  uint4 u = *reinterpret_cast<const uint4*>(base + byte_off);
  return __builtin_bit_cast(typename P::vec8, u);
}

// ---------------------------------------------------------------------------------------------
// Full-line epilogue stores.  After the swapped-operand MFMA, lane (j = lane&15, g = lane>>4) holds two 16-byte
// chunks of pixel/row j: A = bytes [g*16, +16) and B = bytes [64 + g*16, +16) of that pixel's 128-byte feature run.
// Storing A then B makes every store instruction touch 16 different 128-byte lines, half a line each (measured:
// the conv epilogue alone ran at ~1 TB/s).  One DPP row-rotate by 8 swaps chunks between lanes j and j^8 so that
//   r1 of lane j goes to pixel (j & 7)     at byte (j < 8 ? 0 : 64) + g*16
//   r2 of lane j goes to pixel 8 + (j & 7) at the same byte offset
// i.e. each store instruction now writes 8 complete 128-byte lines.
__device__ __forceinline__ uint32_t dpp_ror8(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128 /* row_ror:8 */, 0xF, 0xF, false);
}
__device__ __forceinline__ void line_exchange(uint4& a, uint4& b, int l15) {
  const bool lo = l15 < 8;
  const uint4 x = lo ? b : a;
  uint4 y;
  y.x = dpp_ror8(x.x); y.y = dpp_ror8(x.y); y.z = dpp_ror8(x.z); y.w = dpp_ror8(x.w);
  if (lo) b = y; else { a = y; }
}
// after line_exchange: for lanes >= 8 `a` holds the partner pixel's B chunk and `b` its own B; see call sites

// Reductions across the four 16-lane rows of a wave (lane ^ 16, lane ^ 32) on the VALU: gfx950's v_permlane16_swap /
// v_permlane32_swap exchange rows (halves) between two registers, so swap(x, x) leaves the two partners of every lane side
// by side — one swap + one op instead of a ds_bpermute round trip through the LDS crossbar (~100 cycles of latency each).
__device__ __forceinline__ float rows_max(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const float m = fmaxf(__builtin_bit_cast(float, (unsigned)a[0]), __builtin_bit_cast(float, (unsigned)a[1]));
  const unsigned um = __builtin_bit_cast(unsigned, m);
  const auto b = __builtin_amdgcn_permlane16_swap(um, um, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned)b[0]), __builtin_bit_cast(float, (unsigned)b[1]));
}
__device__ __forceinline__ float rows_sum(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const float m = __builtin_bit_cast(float, (unsigned)a[0]) + __builtin_bit_cast(float, (unsigned)a[1]);
  const unsigned um = __builtin_bit_cast(unsigned, m);
  const auto b = __builtin_amdgcn_permlane16_swap(um, um, false, false);
  return __builtin_bit_cast(float, (unsigned)b[0]) + __builtin_bit_cast(float, (unsigned)b[1]);
}

// LightGlue rotary embedding on the four (even, odd) pairs of v[0..7]: one definition for every GEMM epilogue, so that the
// kernels launch_gemm may pick for the same linear stay bit-identical.
//
// Written as SINGLE v_mul_f32 / v_fma_f32 instructions on purpose.  From the plain C form hipcc's vectoriser makes v_pk_mul_f32 /
// v_pk_fma_f32, and for pair 1 — whose cos / sin sit in the HIGH half of a register pair — with op_sel cross selections
// (`v_pk_mul_f32 .. op_sel:[1,1] op_sel_hi:[0,1]`, `v_pk_fma_f32 .. op_sel:[0,1,0] neg_lo:[0,0,1] neg_hi:[0,0,1]`).  Exactly that
// element (feature 8 g + 2 of a lane's run: the EVEN element of pair 1, lanes 48-63 only, its odd partner right) came out wrong
// in one 16-token tile of the first layer's q | k projection in 0.13 % of the 64-pair steps on a quiet GPU and in 4 % with another
// stream's kernels beside it: the round-2 "matcher race" (tools/experiments/matcher_trace.py names the launch, the tile and the
// element; profiles/r03_matcher_trace_probe1.txt, _probe2.txt).  The same element failed in lg_blockf's folded projection in round 2, where the
// tables came from global loads instead of LDS.  No missing wait count or documented hazard in the ISA; the products and sums
// below are the same ones in the same order, so the bits do not change.
__device__ __forceinline__ void rotate_pairs(float* v, const f32x4& c, const f32x4& s) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float t0, t1, r0, r1;
    asm("v_mul_f32 %0, %1, %2" : "=v"(t0) : "v"(v[2 * i + 1]), "v"(s[i]));
    asm("v_fma_f32 %0, %1, %2, -%3" : "=v"(r0) : "v"(v[2 * i]), "v"(c[i]), "v"(t0));
    asm("v_mul_f32 %0, %1, %2" : "=v"(t1) : "v"(v[2 * i]), "v"(s[i]));
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r1) : "v"(v[2 * i + 1]), "v"(c[i]), "v"(t1));
    v[2 * i] = r0;
    v[2 * i + 1] = r1;
  }
}

}  // namespace airfe
