// airfe — the streaming K = 256 GEMM's workgroup body (see kernels_gemmr.hip for the design): shared by the translation units that instantiate it —
// kernels_gemmr.hip (the matcher's linears, the gather form) and kernels_gemmr_sample.hip (the gather form with the descriptor sampling in its epilogue,
// compiled like kernels_img.hip so that sample_desc_row is the same instructions in both places).
#pragma once
#include "common.h"
#include "kernels.h"
#include "desc_sample.h"

namespace airfe {

constexpr int GR_MT = 2;                          // 16-token MFMA tiles per streamed tile
constexpr int GR_TT = 16 * GR_MT;                 // 32 tokens
constexpr int GR_XBYTES = GR_TT * 512;            // [32][256] 2-byte = 16 KiB
constexpr int GR_RBYTES = 2 * GR_TT * 128;        // cos | sin rows of the tile's tokens, [32][32] fp32 each = 8 KiB

template <int N>
__device__ __forceinline__ void gr_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

__device__ __forceinline__ void gr_glds16(const void* gsrc, unsigned lds_off) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_off)
               : "memory");
}

// One workgroup's whole launch: 256-feature slice `group` of linear `a`, token tiles first, first + per_group, ...
constexpr int GR_SAMPLE_SLOTS = 7;                // SAMPLE: ring slots beside the staging tile
constexpr int GR_STAGE_LD = 260;                  // SAMPLE: floats per staged row (256 + 4: the 16 rows a b128 write touches start 4 banks apart)
constexpr int GR_STAGE_BYTES = GR_TT * GR_STAGE_LD * 4;
struct GrKeypoint { float x, y; int row, second; };   // SAMPLE: one keypoint slot of a tile: feature row of destination 0 / 1; row < 0: nothing to write (k >= n[b], or the padded tail)

// JUNC (DescSample::junc): the tiles of the live prefix — every wave reads the B counts itself (no LDS, no barrier: the result is the same in every wave, so the
// whole workgroup leaves or stays) and the tile count stops at ceil(max n[b] / 8) * B
__device__ __forceinline__ int gr_junc_live_tiles(const DescSample& ds, int ntiles) {
  int kmax = 0;
  for (int b = threadIdx.x & 63; b < ds.B; b += 64) kmax = max(kmax, min(ds.n[b], ds.cap));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o));
  kmax = __builtin_amdgcn_readfirstlane(kmax);
  return min(ntiles, ((kmax + 7) >> 3) * ds.B);
}

template <class P, bool TRANS, bool ROT, bool GATHER = false, bool SAMPLE = false, bool JUNC = false>
__device__ __forceinline__ void gemmr_body(const GemmArgs& a, char* smem, int group, int first, int per_group, int ntiles, const DescSample* dsp = nullptr) {
  static_assert(!GATHER || (!TRANS && !ROT), "the gather form is the plain K = 256 linear with fp32 rows out");
  static_assert(!SAMPLE || GATHER, "sampling finishes the gather form's rows");
  static_assert(!JUNC || SAMPLE, "the junction layout is a slot layout of the sampling form");
  if constexpr (JUNC) ntiles = gr_junc_live_tiles(*dsp, ntiles);       // (before any DMA and any barrier; the ring's wait counts below depend on n only)
  constexpr int GR_SLOT = GR_XBYTES + (ROT ? GR_RBYTES : 0);
  constexpr int GR_SLOTS = ROT ? 6 : SAMPLE ? GR_SAMPLE_SLOTS : 8;
  constexpr int PER = ROT ? 3 : 2;                                    // DMA instructions per wave and tile
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = first < ntiles ? (ntiles - first + per_group - 1) / per_group : 0;
  if (n == 0) return;

  // ---- this wave's weights: feature block cb, tile pair tp -> 16 fragments
  const int cb = group * 4 + (wave >> 1), tp = wave & 1;
  typename P::vec8 wreg[2][8];
  {
    const int sw = (l15 >> 1) & 7;
    const char* wb = reinterpret_cast<const char*>(a.Wp) + (size_t)cb * 4 * SLAB_BYTES + 2 * tp * 2048 + l15 * 128;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
        wreg[u][ks] = __builtin_bit_cast(typename P::vec8, *reinterpret_cast<const uint4*>(
            wb + u * 2048 + (ks >> 1) * SLAB_BYTES + ((((ks & 1) * 4 + g) ^ sw) << 4)));
  }
  f32x4 binit[2];                                                     // !TRANS: bias of the lane's 8 features
  float bt[2];                                                        // TRANS: bias of the lane's feature column per tile
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    binit[u] = *reinterpret_cast<const f32x4*>(a.bias + cb * 64 + tp * 32 + g * 8 + u * 4);
    bt[u] = a.bias[cb * 64 + slab_row_to_feature((2 * tp + u) * 16 + l15)];
  }
  // GATHER: the source rows of every tile this workgroup will stream, [n][32] behind the ring
  [[maybe_unused]] float* stage = reinterpret_cast<float*>(smem + GR_SLOTS * GR_SLOT);      // SAMPLE: [32][GR_STAGE_LD] fp32, the tile's head rows
  [[maybe_unused]] int* idx_lds = reinterpret_cast<int*>(smem + GR_SLOTS * GR_SLOT + (SAMPLE ? GR_STAGE_BYTES : 0));
  [[maybe_unused]] GrKeypoint* kp_lds = reinterpret_cast<GrKeypoint*>(idx_lds + n * GR_TT);   // SAMPLE: [n][8] (16-byte entries behind the 128-byte index rows)
  if constexpr (GATHER && !JUNC) {       // (a.rowidx == nullptr: the identity — every row in order, fp32 rows out: the DENSE descriptor head of the junction images)
    for (int e = tid; e < n * GR_TT; e += 512) {
      const int r = (first + (e >> 5) * per_group) * GR_TT + (e & 31);
      idx_lds[e] = a.rowidx ? a.rowidx[r] : r;
    }
  }
  if constexpr (JUNC) {         // tile T = slots 8 (T / B) .. + 7 of image T % B; the slot's four tap rows from its x, y (desc_taps, as the epilogue calls it): no row list in memory
    const DescSample& ds = *dsp;
    const int cells = ds.HC * ds.WC;
    for (int e = tid; e < n * 8; e += 512) {
      const int T = first + (e >> 3) * per_group;
      const int b = T % ds.B, k = (T / ds.B) * 8 + (e & 7);
      GrKeypoint kp{0.f, 0.f, -1, 0};
      int r0 = 0, r1 = 0, r2 = 0, r3 = 0;                               // a dead slot gathers row 0 and writes nothing
      if (k < ds.cap && k < ds.n[b]) {
        const float* f = ds.feat + ((size_t)b * ds.cap + k) * 259;
        kp.row = b * ds.cap + k;
        kp.x = f[1];
        kp.y = f[2];
        const DescTaps t = desc_taps(kp.x, kp.y, ds.sx, ds.bx, ds.sy, ds.by, ds.HC, ds.WC);
        r0 = b * cells + t.c[0]; r1 = b * cells + t.c[1]; r2 = b * cells + t.c[2]; r3 = b * cells + t.c[3];
      }
      kp_lds[e] = kp;
      *reinterpret_cast<int4*>(idx_lds + e * 4) = make_int4(r0, r1, r2, r3);
    }
  } else if constexpr (SAMPLE) {       // keypoint slot s = row / 4 = b * cap + k over ALL images of the launch; the two destinations split at image Bs
    const DescSample& ds = *dsp;
    for (int e = tid; e < n * 8; e += 512) {
      const int s = (first + (e >> 3) * per_group) * 8 + (e & 7);
      const int b = s / ds.cap, k = s - b * ds.cap;
      GrKeypoint kp{0.f, 0.f, -1, 0};
      if (b < ds.B) {
        const bool second = ds.feat1 && b >= ds.Bs;
        const int bl = second ? b - ds.Bs : b;
        if (k < (second ? ds.n1 : ds.n)[bl]) {
          const float* f = (second ? ds.feat1 : ds.feat) + ((size_t)bl * ds.cap + k) * 259;
          kp.row = bl * ds.cap + k;
          kp.second = second ? 1 : 0;
          kp.x = f[1];
          kp.y = f[2];
        }
      }
      kp_lds[e] = kp;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (GATHER) __syncthreads();

  // ---- DMA of the workgroup's j-th tile (t = first + j per_group; 32 rows x 512 B) into ring slot `slot`: 16 wave-instructions of 1 KiB, two per wave, two rows each
  const int ld = a.ld1;
  auto dma = [&](int j, int slot) {
    [[maybe_unused]] const int t = first + j * per_group;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int inst = wave * 2 + i;
      const int r = inst * 2 + (lane >> 5), pp = lane & 31;
      size_t srow;
      if constexpr (GATHER) srow = (size_t)idx_lds[j * GR_TT + r];
      else srow = (size_t)(t * GR_TT + r);
      gr_glds16(a.X1 + srow * ld + ((pp ^ (r & 15)) << 3), (unsigned)(slot * GR_SLOT + inst * 1024));
    }
    if constexpr (ROT) {                                              // waves 0-3: cos rows, 4-7: sin rows; 8 rows of 128 B per instruction
      const float* src = (wave < 4 ? a.rot_cos : a.rot_sin) + ((size_t)t * GR_TT + (wave & 3) * 8) * 32 + lane * 4;
      gr_glds16(src, (unsigned)(slot * GR_SLOT + GR_XBYTES + wave * 1024));
    }
  };
#pragma unroll
  for (int j = 0; j < GR_SLOTS; ++j)
    if (j < n) dma(j, j);
  // tile 0 landed: at most PER * min(n - 1, GR_SLOTS - 1) younger DMA instructions may still be in flight
  if (n >= GR_SLOTS) gr_wait_vm<PER * (GR_SLOTS - 1)>();
  else gr_wait_vm<0>();
  __syncthreads();

  const int boff0 = l15 * 512;
  for (int i = 0; i < n; ++i) {
    const int t = first + i * per_group, slot = i % GR_SLOTS;          // (six slots with rotary: not a power of two)
    const char* xs = smem + slot * GR_SLOT + boff0;
    f32x4 acc[2][GR_MT];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int m = 0; m < GR_MT; ++m) acc[u][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      typename P::vec8 bf[GR_MT];
#pragma unroll
      for (int m = 0; m < GR_MT; ++m) bf[m] = lds_frag<P>(xs, m * 16 * 512 + (((ks * 4 + g) ^ l15) << 4));
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int m = 0; m < GR_MT; ++m) {
          if constexpr (TRANS) acc[u][m] = P::mfma(bf[m], wreg[u][ks], acc[u][m]);
          else acc[u][m] = P::mfma(wreg[u][ks], bf[m], acc[u][m]);
        }
    }
    // tile i+1 landed (this wave's part): behind it at most the tiles i+2 .. i+GR_SLOTS-1 are in flight, PER instructions each
    const int behind = n - 2 - i;
    if (behind >= GR_SLOTS - 2) gr_wait_vm<PER * (GR_SLOTS - 2)>();
    else if (behind == 5) gr_wait_vm<PER * 5>();
    else if (behind == 4) gr_wait_vm<PER * 4>();
    else if (behind == 3) gr_wait_vm<PER * 3>();
    else if (behind == 2) gr_wait_vm<PER * 2>();
    else if (behind == 1) gr_wait_vm<PER>();
    else gr_wait_vm<0>();

    // ---- epilogue of tile i (stores only)
    if constexpr (!TRANS) {
      const int co = cb * 64 + tp * 32 + g * 8;
#pragma unroll
      for (int m = 0; m < GR_MT; ++m) {
        const int row = t * GR_TT + m * 16 + l15;
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[0][m][e] + binit[0][e];          // bias after the K sum, like the tiled kernels: bit-identical results
          v[4 + e] = acc[1][m][e] + binit[1][e];
        }
        if constexpr (ROT) {                                          // rotary on the pairs (2i, 2i+1) of the head dimension: light_glue rotary, as gemm_store_run
          const char* rt = smem + slot * GR_SLOT + GR_XBYTES + (m * 16 + l15) * 128 + (tp * 16 + g * 4) * 4;
          const f32x4 cs = *reinterpret_cast<const f32x4*>(rt), sn = *reinterpret_cast<const f32x4*>(rt + GR_RBYTES / 2);
          rotate_pairs(v, cs, sn);
        }
        if constexpr (SAMPLE) {                                       // the same values, to the staging tile
          float* o = stage + (m * 16 + l15) * GR_STAGE_LD + co;
          *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
          *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else if constexpr (GATHER) {                                // EPI_STORE_F32: the lane's 8 features of output row `row` (dense row order, not the source's)
          float* o = reinterpret_cast<float*>(a.out) + (size_t)row * a.ldo + co;
          *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
          *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else if (a.epi == EPI_HEADS) {
          const int s = row / a.Np, nn = row - s * a.Np;
          const int sel = co >> 8, cw = co & 255, h = cw >> 6, d = cw & 63;
          uint16_t* o = reinterpret_cast<uint16_t*>(sel ? a.out2 : a.out) + (((size_t)s * a.H + h) * a.Np + nn) * 64 + d;
          *reinterpret_cast<uint4*>(o) = pack8<P>(v);
        } else {                                                      // EPI_STORE
          *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(a.out) + (size_t)row * a.ldo + co) = pack8<P>(v);
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int co = cb * 64 + slab_row_to_feature((2 * tp + u) * 16 + l15);
        const int h = co >> 6, d = co & 63;
#pragma unroll
        for (int m = 0; m < GR_MT; ++m) {
          const int row0 = t * GR_TT + m * 16 + g * 4;
          const int sq = row0 / a.Np, nn = row0 - sq * a.Np;
          uint16_t* o = reinterpret_cast<uint16_t*>(a.out) + (((size_t)sq * a.H + h) * 64 + d) * a.Np + nn;
          *reinterpret_cast<uint2*>(o) = pack4<P>(acc[u][m][0] + bt[u], acc[u][m][1] + bt[u], acc[u][m][2] + bt[u], acc[u][m][3] + bt[u]);
        }
      }
    }
    __syncthreads();                                                  // every wave is done with slot i and has its part of tile i+1
    if (i + GR_SLOTS < n) dma(i + GR_SLOTS, slot);
    if constexpr (SAMPLE) {                                           // (behind the barrier: the staged tile is complete) wave w finishes keypoint w of the tile
      const DescSample& ds = *dsp;
      const GrKeypoint kp = kp_lds[i * 8 + wave];
      if (kp.row >= 0) {                                              // wave-uniform
        float* f = (kp.second ? ds.feat1 : ds.feat) + (size_t)kp.row * 259;
        const DescTaps tp = desc_taps(kp.x, kp.y, ds.sx, ds.bx, ds.sy, ds.by, ds.HC, ds.WC);
        const float* d = stage + (wave * 4) * GR_STAGE_LD + lane * 4;
        const float4 a0 = *reinterpret_cast<const float4*>(d), a1 = *reinterpret_cast<const float4*>(d + GR_STAGE_LD);
        const float4 a2 = *reinterpret_cast<const float4*>(d + 2 * GR_STAGE_LD), a3 = *reinterpret_cast<const float4*>(d + 3 * GR_STAGE_LD);
        sample_desc_row(a0, a1, a2, a3, tp, kp.x, kp.y, f, lane, 1, ds.w_scale, ds.h_scale, ds.flag);
      }
      __syncthreads();                                                // the staging tile is free for tile i+1's values
    }
  }
}

}  // namespace airfe
