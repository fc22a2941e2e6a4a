// airfe — stereo line triangulation: the loop of Frame::AddRightFeatures over the line matches (src/frame.cc:185-191), TriangulateByStereo
// (src/line_processor.cc:196-245) with Camera::BackProjectStereo (src/camera.cc:268-280), and ComputeLine3DFromEndpoints (src/line_processor.cc:312-326)
// as Mapline::SetEndpoints calls it (src/mapline.cc:74-83), on plain arrays.  Contract: include/airfe.h ("Stereo lines").  One statement for the host and
// the device: the kernel (kernels_stereoline.hip) calls sl_line from its lanes, stereoline_host at the end calls it in a loop; tests/stereoline_ref.py
// restates the same with Python floats.  Doubles only; no fused multiply-add on either side (the translation unit that includes this is compiled with
// -ffp-contract=off); every sum is written in the order it is evaluated in; the only non-rational function is sqrt.
#ifndef AIRFE_STEREOLINE_CORE_H_
#define AIRFE_STEREOLINE_CORE_H_

#include <math.h>
#include <stdint.h>

#include "core_common.h"

// The reference's gate is |atan(dy / dx)| < 0.175; an atan evaluated by two libms is two functions.  atan is monotone, so the gate is |dy / dx| < t with
// t the smallest double whose atan is >= 0.175: 0x1.6a1aa2e1bef6fp-3 (= tan(0.175) rounded; tests/test_stereoline_cpu.py finds it again by bisection on
// the host's atan and sweeps its neighbourhood).
#define SL_TAN_GATE 0x1.6a1aa2e1bef6fp-3
#define SL_MIN_LENGTH 0.01            // line_processor.cc:317

enum {
  SL_OK = 0,                          // a map line: endpoints and Pluecker line set
  SL_NO_RIGHT = 1,                    // no right line (frame.cc:186)
  SL_LEFT_HORIZONTAL = 2,             // line_processor.cc:211
  SL_RIGHT_HORIZONTAL = 3,            // :216
  SL_DISPARITY = 4,                   // :232
  SL_SHORT = 5                        // triangulated, |p2 - p1| < 0.01 (:317): endpoints set, no Pluecker line
};


// frame.cc:186 — `> 0` is the reference's: a match to right line 0 is dropped.  r >= nr (a stale index) is invalid and never indexes memory.
AIRFE_HD bool sl_right_valid(int r, int nr) { return r > 0 && r < nr; }

// line_processor.cc:210-211 / :215-216.  dx == 0: dy / dx = +-inf, not below the gate (atan = +-pi/2); dx == dy == 0: NaN, already horizontal by |dy| <= 3.
AIRFE_HD bool sl_horizontal(double dx, double dy) { return fabs(dy) <= 3.0 || fabs(dy / dx) < SL_TAN_GATE; }

AIRFE_HD void sl_nan(double* v, int n) {
  for (int k = 0; k < n; ++k) v[k] = quiet_nan();
}

// Camera::BackProjectStereo on (x, y, x_right): ((x - cx) fx_inv, (y - cy) fy_inv, 1) * (bf / (x - x_right))
AIRFE_HD void sl_back_project(double x, double y, double x_right, double bf, double fx_inv, double fy_inv, double cx, double cy, double* p) {
  const double d = bf / (x - x_right);
  p[0] = ((x - cx) * fx_inv) * d;
  p[1] = ((y - cy) * fy_inv) * d;
  p[2] = 1.0 * d;
}

// Rwc p + twc, Twc row-major [16]: each row ((r0 x + r1 y) + r2 z) + t.  Twc == nullptr: p stays as it is, nothing is multiplied.
AIRFE_HD void sl_to_world(const double* Twc, double* p) {
  if (!Twc) return;
  const double x = p[0], y = p[1], z = p[2];
  for (int r = 0; r < 3; ++r) p[r] = ((Twc[4 * r] * x + Twc[4 * r + 1] * y) + Twc[4 * r + 2] * z) + Twc[4 * r + 3];
}

// ComputeLine3DFromEndpoints with g2o::Line3D::fromCartesian written out (the formula here is the contract): l = p2 - p1, d = l / |l|,
// p = p1 - d (d . p1), w = p x (p + d); plucker = (w, d).  false (and NaN) when |l| < 0.01.
AIRFE_HD bool sl_plucker(const double* e, double* plucker) {
  const double lx = e[3] - e[0], ly = e[4] - e[1], lz = e[5] - e[2];
  const double n = sqrt((lx * lx + ly * ly) + lz * lz);
  if (n < SL_MIN_LENGTH) {
    sl_nan(plucker, 6);
    return false;
  }
  const double dx = lx / n, dy = ly / n, dz = lz / n;
  const double dot = (dx * e[0] + dy * e[1]) + dz * e[2];
  const double px = e[0] - dx * dot, py = e[1] - dy * dot, pz = e[2] - dz * dot;
  const double qx = px + dx, qy = py + dy, qz = pz + dz;
  plucker[0] = py * qz - pz * qy;
  plucker[1] = pz * qx - px * qz;
  plucker[2] = px * qy - py * qx;
  plucker[3] = dx; plucker[4] = dy; plucker[5] = dz;
  return true;
}

// One left line with its selected right line.  cam [8] = min_x_diff, max_x_diff, max_y_diff (unused), bf, fx, fy, cx, cy.  endpoints [6] and
// plucker [6] are always written (NaN where the status says they are not set).  Returns the status.
AIRFE_HD int sl_line(const double* cam, const double* left, const double* right, bool valid, const double* Twc, double* endpoints, double* plucker) {
  sl_nan(endpoints, 6);
  sl_nan(plucker, 6);
  if (!valid) return SL_NO_RIGHT;
  const double x11 = left[0], y11 = left[1], x12 = left[2], y12 = left[3];
  const double x21 = right[0], y21 = right[1], x22 = right[2], y22 = right[3];
  const double dx_left = x12 - x11, dy_left = y12 - y11;
  if (sl_horizontal(dx_left, dy_left)) return SL_LEFT_HORIZONTAL;
  const double dx_right = x22 - x21, dy_right = y22 - y21;
  if (sl_horizontal(dx_right, dy_right)) return SL_RIGHT_HORIZONTAL;
  const double k_inv_right = dx_right / dy_right;
  const double x11_right = x21 + k_inv_right * (y11 - y21);
  const double x12_right = x21 + k_inv_right * (y12 - y21);
  const double dx1 = x11 - x11_right, dx2 = x12 - x12_right;
  const double min_x_diff = cam[0], max_x_diff = cam[1];
  if (dx1 < min_x_diff || dx1 > max_x_diff || dx2 < min_x_diff || dx2 > max_x_diff) return SL_DISPARITY;
  const double fx_inv = 1.0 / cam[4], fy_inv = 1.0 / cam[5];
  sl_back_project(x11, y11, x11_right, cam[3], fx_inv, fy_inv, cam[6], cam[7], endpoints);
  sl_back_project(x12, y12, x12_right, cam[3], fx_inv, fy_inv, cam[6], cam[7], endpoints + 3);
  sl_to_world(Twc, endpoints);
  sl_to_world(Twc, endpoints + 3);
  return sl_plucker(endpoints, plucker) ? SL_OK : SL_SHORT;
}

// Line i of a frame: selection (frame.cc:185-191), then sl_line.  sel [4], *flag, *status, endpoints [6], plucker [6] are this line's slots.
AIRFE_HD int sl_frame_line(const double* cam, const double* lines_left, const double* lines_right, int nr, const int32_t* matches, const double* Twc, int i,
                        double* sel, uint8_t* flag, int32_t* status, double* endpoints, double* plucker) {
  const int r = matches[i];
  const bool valid = sl_right_valid(r, nr);
  for (int k = 0; k < 4; ++k) sel[k] = valid ? lines_right[(size_t)r * 4 + k] : 0.0;
  *flag = valid ? 1 : 0;
  const int s = sl_line(cam, lines_left + (size_t)i * 4, sel, valid, Twc, endpoints, plucker);
  *status = s;
  return s;
}

// The host statement over ONE frame: lines_left [nl][4], lines_right [nr][4], matches [nl], Twc [16] or nullptr; the outputs' first nl slots are
// written; count [3] = valid right lines, status 0 or 5, status 0.
inline void stereoline_host(const double* cam, const double* lines_left, int nl, const double* lines_right, int nr, const int32_t* matches, const double* Twc,
                            double* sel, uint8_t* flag, int32_t* status, double* endpoints, double* plucker, int32_t* count) {
  count[0] = count[1] = count[2] = 0;
  for (int i = 0; i < nl; ++i) {
    const int s = sl_frame_line(cam, lines_left, lines_right, nr, matches, Twc, i, sel + (size_t)i * 4, flag + i, status + i, endpoints + (size_t)i * 6,
                                plucker + (size_t)i * 6);
    count[0] += s != SL_NO_RIGHT;
    count[1] += s == SL_OK || s == SL_SHORT;
    count[2] += s == SL_OK;
  }
}

#endif  // AIRFE_STEREOLINE_CORE_H_
