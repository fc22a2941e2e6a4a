// airfe — batched stereo line triangulation on the device: the matched stereo line pairs of B keyframes to 3-D endpoints and Pluecker lines
// (Frame::AddRightFeatures' loop over the line matches, src/frame.cc:185-191; TriangulateByStereo, src/line_processor.cc:196-245;
// ComputeLine3DFromEndpoints, :312-326).  Contract: include/airfe.h ("Stereo lines").  The rules are stereoline_core.h's, shared with the host statement;
// the file is compiled with -ffp-contract=off.
//   stereoline_kernel   one launch over all B x capL line slots, one lane per line: a few dozen fp64 operations behind five loads, latency-bound; no LDS,
//                       no scratch.  blockIdx.y = the frame, so a wave never spans two frames: the three counts are a ballot per wave and one integer
//                       atomicAdd per wave and count (integer sums: the same bytes in every run)
#include "kernels.h"
#include "stereoline_core.h"

namespace airfe {

namespace {

__global__ __launch_bounds__(256) void stereoline_kernel(StereoLineArgs a) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int nl = clamp_count(a.nl[b], a.capL), nr = clamp_count(a.nr[b], a.capL);
  const bool live = i < nl;
  int s = -1;
  if (live) {
    const size_t o = (size_t)b * a.capL;
    double sel[4], e[6], p[6];
    uint8_t flag;
    int32_t status;
    s = sl_frame_line(a.cam, a.left + o * 4, a.right + o * 4, nr, a.matches + o, a.Twc ? a.Twc + (size_t)b * 16 : nullptr, i, sel, &flag, &status, e, p);
    double* ds = a.sel + (o + i) * 4;
    double* de = a.endpoints + (o + i) * 6;
    double* dp = a.plucker + (o + i) * 6;
    for (int k = 0; k < 4; ++k) ds[k] = sel[k];
    for (int k = 0; k < 6; ++k) de[k] = e[k];
    for (int k = 0; k < 6; ++k) dp[k] = p[k];
    a.valid[o + i] = flag;
    a.status[o + i] = status;
  }
  const int n_valid = __popcll(__ballot(live && s != SL_NO_RIGHT));
  const int n_tri = __popcll(__ballot(live && (s == SL_OK || s == SL_SHORT)));
  const int n_ok = __popcll(__ballot(live && s == SL_OK));
  if ((threadIdx.x & 63) == 0) {
    if (n_valid) atomicAdd(&a.count[3 * b], n_valid);
    if (n_tri) atomicAdd(&a.count[3 * b + 1], n_tri);
    if (n_ok) atomicAdd(&a.count[3 * b + 2], n_ok);
  }
}

}  // namespace

void launch_stereo_lines(const StereoLineArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(stereoline_kernel, dim3((a.capL + 255) / 256, B), dim3(256), 0, st, a);
}

void stereo_lines_host(const double* cam, const double* lines_left, int nl, const double* lines_right, int nr, const int32_t* matches, const double* Twc,
                       double* sel, uint8_t* valid, int32_t* status, double* endpoints, double* plucker, int32_t* count) {
  stereoline_host(cam, lines_left, nl, lines_right, nr, matches, Twc, sel, valid, status, endpoints, plucker, count);
}

}  // namespace airfe
