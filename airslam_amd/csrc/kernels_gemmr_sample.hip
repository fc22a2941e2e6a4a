// airfe — the descriptor head over the sampled cells WITH the sampling: the gather form of the streaming GEMM (gemmr_body.h, SAMPLE) finishing eight keypoints
// per 32-row tile from LDS.  A translation unit of its own: built with the flags of kernels_img.hip (no SLP vectoriser), so that sample_desc_row's arithmetic is
// the instruction sequence of sample_desc_kernel — the two are compared byte for byte (tests/test_gpu_detector_tail.py).
#include "gemmr_body.h"

namespace airfe {

// ... with the descriptor sampling in the epilogue (gemmr_body.h, SAMPLE): no head rows in memory
template <class P>
__global__ __launch_bounds__(512, 1) void gemmr_gather_kernel_sample(GemmArgs a, int ntiles, DescSample ds) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemmr_body<P, false, false, true, true>(a, smem, 0, blockIdx.x, gridDim.x, ntiles, &ds);
}

// ... with the junction slot layout (DescSample::junc): an instantiation of its own, so that the point path's kernels above keep their instruction stream
template <class P>
__global__ __launch_bounds__(512, 1) void gemmr_gather_kernel_sample_junc(GemmArgs a, int ntiles, DescSample ds) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemmr_body<P, false, false, true, true, true>(a, smem, 0, blockIdx.x, gridDim.x, ntiles, &ds);
}

constexpr int GR_SAMPLE_MAX_TILES = 60;          // 7 x 16 KiB ring + 32.5 KiB staging tile + 256 B per tile (row list, keypoint list) <= 160 KiB
bool gemmr_gather_sample_applicable(const GemmArgs& a) {
  const int wgs = std::max(a.gr_wgs, 1);
  return gemmr_gather_applicable(256, a) && a.rowidx && (a.M / GR_TT + wgs - 1) / wgs <= GR_SAMPLE_MAX_TILES;
}

void launch_gemmr_gather_sample(int prec, const GemmArgs& a, const DescSample& ds0, hipStream_t st) {
  DescSample ds = ds0;
  desc_grid_coeffs(ds.HC, ds.WC, ds.sx, ds.bx, ds.sy, ds.by);
  const int ntiles = a.M / GR_TT;
  const int nwg = std::max(std::min(a.gr_wgs, ntiles), 1);
  const int nmax = (ntiles + nwg - 1) / nwg;
  const int lds = GR_SAMPLE_SLOTS * GR_XBYTES + GR_STAGE_BYTES + nmax * (GR_TT * 4 + 8 * (int)sizeof(GrKeypoint));
  if (prec == 1) {
    static PerDeviceOnce once;
    if (auto once_token = once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemmr_gather_kernel_sample<PF16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(gemmr_gather_kernel_sample<PF16>, dim3((unsigned)nwg), dim3(512), lds, st, a, ntiles, ds);
  } else {
    static PerDeviceOnce once;
    if (auto once_token = once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemmr_gather_kernel_sample<PBF16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(gemmr_gather_kernel_sample<PBF16>, dim3((unsigned)nwg), dim3(512), lds, st, a, ntiles, ds);
  }
}

// The junction layout: a.M is the untrimmed bound ceil(cap / 8) * B tiles of 32 rows (LDS is sized by it; the workgroups trim themselves to the live prefix)
bool gemmr_gather_sample_junc_applicable(const GemmArgs& a, const DescSample& ds) {
  const int wgs = std::max(a.gr_wgs, 1);
  return gemmr_gather_applicable(256, a) && !a.rowidx && ds.junc && !ds.feat1 && ds.B >= 1 && ds.cap >= 1 && a.M == (ds.cap + 7) / 8 * ds.B * GR_TT &&
         (a.M / GR_TT + wgs - 1) / wgs <= GR_SAMPLE_MAX_TILES;
}

void launch_gemmr_gather_sample_junc(int prec, const GemmArgs& a, const DescSample& ds0, hipStream_t st) {
  DescSample ds = ds0;
  desc_grid_coeffs(ds.HC, ds.WC, ds.sx, ds.bx, ds.sy, ds.by);
  const int ntiles = a.M / GR_TT;
  const int nwg = std::max(std::min(a.gr_wgs, ntiles), 1);
  const int nmax = (ntiles + nwg - 1) / nwg;
  const int lds = GR_SAMPLE_SLOTS * GR_XBYTES + GR_STAGE_BYTES + nmax * (GR_TT * 4 + 8 * (int)sizeof(GrKeypoint));
  if (prec == 1) {
    static PerDeviceOnce once;
    if (auto once_token = once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemmr_gather_kernel_sample_junc<PF16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(gemmr_gather_kernel_sample_junc<PF16>, dim3((unsigned)nwg), dim3(512), lds, st, a, ntiles, ds);
  } else {
    static PerDeviceOnce once;
    if (auto once_token = once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemmr_gather_kernel_sample_junc<PBF16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(gemmr_gather_kernel_sample_junc<PBF16>, dim3((unsigned)nwg), dim3(512), lds, st, a, ntiles, ds);
  }
}

}  // namespace airfe
