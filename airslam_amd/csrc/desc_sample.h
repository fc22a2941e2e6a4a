// airfe — descriptor sampling shared by the kernels that run it: the four bilinear taps of a keypoint (desc_taps) and the finish of one
// keypoint from its four head rows (sample_desc_row).  sample_desc_kernel (kernels_img.hip) reads the rows from memory, the fused gather
// GEMM (kernels_gemmr_sample.hip) from the LDS tile it has just computed, and select_list_kernel (kernels_sel.hip) writes the tap rows the
// GEMM gathers: ONE statement of the arithmetic, so the same floats give the same bits wherever it runs.
#pragma once
#include <cfloat>

#include "common.h"
#include "wg_prims.h"

namespace airfe {

// extract_descriptors (src/plnet.cpp:369-417 == src/super_point.cpp:224-272).
// Contraction is SPELLED OUT here: hipcc's __fmul_rn / __fadd_rn are plain operators compiled with contraction allowed, which the compiler fuses into fmas as it
// sees fit — differently from one kernel to the next (inlined elsewhere, the same source gave x*x + .. in another association and ix_se - kx * (WC - 1) as one fma).
// So every function below runs with contraction off, uses the plain operators (the pragma does not reach into the header's intrinsics) and states its fmas
// itself, in the form sample_desc_kernel has always been compiled to: the bits do not depend on which kernel the code is inlined into.
__device__ __forceinline__ int clipi(int v, int mx) { return v < 0 ? 0 : min(v, mx - 1); }

// the four taps of a keypoint (grid_sample bilinear, align_corners semantics of extract_descriptors) and their weights
struct DescTaps { int c[4]; float w[4]; };       // cell = iy * WC + ix of nw, ne, sw, se
__device__ __forceinline__ DescTaps desc_taps(float x, float y, float sx, float bx, float sy, float by, int HC, int WC) {
#pragma clang fp contract(off)
  float kx = __builtin_fmaf(x, sx, bx), ky = __builtin_fmaf(y, sy, by);
  kx = (kx + 1.0f) * 0.5f;
  ky = (ky + 1.0f) * 0.5f;
  const float ix = kx * (float)(WC - 1), iy = ky * (float)(HC - 1);
  const int ix_nw = clipi((int)floorf(ix), WC), iy_nw = clipi((int)floorf(iy), HC);
  const int ix_ne = clipi(ix_nw + 1, WC), iy_ne = clipi(iy_nw, HC);
  const int ix_sw = clipi(ix_nw, WC), iy_sw = clipi(iy_nw + 1, HC);
  const int ix_se = clipi(ix_nw + 1, WC), iy_se = clipi(iy_nw + 1, HC);
  DescTaps t;
  t.w[0] = ((float)ix_se - ix) * ((float)iy_se - iy);
  t.w[1] = (ix - (float)ix_sw) * ((float)iy_sw - iy);
  t.w[2] = ((float)ix_ne - ix) * (iy - (float)iy_ne);
  t.w[3] = (ix - (float)ix_nw) * (iy - (float)iy_nw);
  t.c[0] = iy_nw * WC + ix_nw; t.c[1] = iy_ne * WC + ix_ne; t.c[2] = iy_sw * WC + ix_sw; t.c[3] = iy_se * WC + ix_se;
  return t;
}

// the keypoint -> normalised grid coordinate coefficients of extract_descriptors (s = 8: the descriptor map's cell size)
static inline void desc_grid_coeffs(int HC, int WC, float& sx, float& bx, float& sy, float& by) {
  const int s = 8;
  sx = (float)(2.0 / (WC * s - s / 2 - 0.5)); bx = (float)((1 - s) / (WC * s - s / 2 - 0.5) - 1);
  sy = (float)(2.0 / (HC * s - s / 2 - 0.5)); by = (float)((1 - s) / (HC * s - s / 2 - 0.5) - 1);
}

// F.normalize(dim=channel) of one 256-channel row spread over a wave, 4 channels per lane
__device__ __forceinline__ void l2norm_lane4(float4& v) {
#pragma clang fp contract(off)
  const float ss = wave_sum(__builtin_fmaf(v.w, v.w, __builtin_fmaf(v.z, v.z, __builtin_fmaf(v.x, v.x, v.y * v.y))));
  const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
  v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
}

// One keypoint, one wave: lane = 4 channels of its four head rows a0 .. a3 (nw, ne, sw, se) -> the descriptor columns 3 .. 258 of feature
// row f, and the final rescale of its x, y (plnet.cpp:574-575).
__device__ __forceinline__ void sample_desc_row(float4 a0, float4 a1, float4 a2, float4 a3, const DescTaps& tp, float x, float y, float* f, int lane,
                                                int normalise, float w_scale, float h_scale, int* flag) {
#pragma clang fp contract(off)
  const float nw = tp.w[0], ne = tp.w[1], sw = tp.w[2], se = tp.w[3];
  if (normalise) {       // F.normalize(dim=channel) of the four cells, operation for operation as l2norm256_kernel does it
    l2norm_lane4(a0);
    l2norm_lane4(a1);
    l2norm_lane4(a2);
    l2norm_lane4(a3);
  }
  float v[4];
  const float n0[4] = {a0.x, a0.y, a0.z, a0.w}, n1[4] = {a1.x, a1.y, a1.z, a1.w};
  const float n2[4] = {a2.x, a2.y, a2.z, a2.w}, n3[4] = {a3.x, a3.y, a3.z, a3.w};
#pragma unroll
  for (int j = 0; j < 4; ++j)          // nw n0 + ne n1 + sw n2 + se n3
    v[j] = __builtin_fmaf(n3[j], se, __builtin_fmaf(n2[j], sw, __builtin_fmaf(n0[j], nw, n1[j] * ne)));
  float ss = __builtin_fmaf(v[3], v[3], __builtin_fmaf(v[2], v[2], __builtin_fmaf(v[0], v[0], v[1] * v[1])));
  ss = wave_sum(ss);
  const float nrm = sqrtf(ss);
  if (flag && lane == 0 && !(ss <= FLT_MAX)) *reinterpret_cast<volatile int*>(flag + 1) = 1;      // inf / NaN descriptor: the detector's 2-byte activations overflowed (airfe.h, "activation range")
  // Eigen (>= 3.3) colwise().normalize(): `if (squaredNorm() > 0) v /= sqrt(squaredNorm())` — a zero column stays zero, no NaN
#pragma unroll
  for (int j = 0; j < 4; ++j) f[3 + lane * 4 + j] = (ss > 0.f) ? v[j] / nrm : v[j];
  if (lane == 0) {
    f[1] = x * w_scale;
    f[2] = y * h_scale;
  }
}

}  // namespace airfe
