// airfe — the positions of a loaded map's points from their observations: Map::TriangulateMappoint (src/map.cc:367-414), the linear multi-view
// triangulation over every observer of a map point, on plain arrays.  Contract: include/airfe.h ("Map-point triangulation").  One statement for the host
// and the device: the kernels (kernels_triangulate.hip) call the routines below from their lanes, triangulate_build_host at the end calls them in loops;
// tests/triangulate_ref.py restates the same in plain Python floats.  Doubles, every sum sequential in the order written, no fused multiply-adds (the
// translation units that include this header are compiled with -ffp-contract=off).
//   observers     valid(f, i) as in covis_core.h (clamp_count, cv_row_id).  The observation of point m in frame f is the FIRST row i of f with valid(f, i)
//                 and id m (cv_first_occurrence).  STATED DIFFERENCE: the reference keeps the last AddObverser per frame.  Observers are taken in
//                 ascending frame index (the reference's std::map order); nobs[m] is their number.
//   per observer  fxi = 1.0 / fx, fyi = 1.0 / fy (Camera::BackProjectMono, camera.cc:268-273); R, c = rotation and translation of the frame's stored Twc
//                   b   = (((double)x - cx) * fxi, ((double)y - cy) * fyi, 1)
//                   v_r = (R[r][0] * b0 + R[r][1] * b1) + R[r][2] * b2
//                   s   = (v0 * v0 + v1 * v1) + v2 * v2          w_r = v_r * (1.0 / s)          d = (v0 * c0 + v1 * c1) + v2 * c2
//                 accumulated in observer order: M[r][q] += w_r * v_q, g_r += w_r * d, C_r += c_r
//   system        A[r][q] = (r == q ? n : 0.0) - M[r][q], rhs_r = C_r - g_r (map.cc:398-403)
//   solve         column-pivoted Householder QR of A by the rules of Eigen's ColPivHouseholderQR as far as they decide anything: the pivot is the remaining
//                 column of largest squared norm over the remaining rows, the first such column wins a tie; the reflector is Eigen's makeHouseholder
//                 (beta = -sign(c0) * sqrt(c0^2 + |tail|^2), essential = tail / (c0 - beta), tau = (beta - c0) / beta; tail^2 <= DBL_MIN: tau = 0,
//                 beta = c0), applied as Eigen's applyHouseholderOnTheLeft (tmp = essential . bottom + top; top -= tau * tmp; bottom -= (tau * essential)
//                 * tmp); rank = #{ |R_kk| > 1e-5 * max_k |R_kk| } (map.cc:405-409); with rank 3: x = P R^-1 Q^T rhs by back substitution.
//                 STATED DIFFERENCES: the remaining column norms are recomputed at every step where Eigen down-dates them; Eigen's count of non-zero
//                 pivots (a column below epsilon times the largest) only ever lowers a rank the 1e-5 rule has already lowered, so it is not restated.
//                 Eigen is not available where this is built and tested: byte equality with Eigen is NOT claimed, only with the statements named above.
//   status        -1 no observer; 0 ok; 1 nobs < max(min_observers, 2); 2 rank < 3; 3 a non-finite keypoint, pose entry (rows 0 .. 2 of Twc), s, system
//                 entry or result, or s == 0, among the point's observers.  Decided in that order of precedence: -1, 1, 3 (observers, system), 2, 3 (result).
//                 xyz = NaN (the quiet NaN 0x7ff8000000000000) unless status is 0.  A point's outputs depend on its own observers only.
#ifndef AIRFE_TRIANGULATE_CORE_H_
#define AIRFE_TRIANGULATE_CORE_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "covis_core.h"

#define TR_MAX_FRAMES CV_MAX_FRAMES  // frames a triangulation handles: (frame, row) packs as f * cap + i into an int32 at 4096 frames x 1024 rows
#define TR_RANK_TOL 1e-5             // kRankLossTolerance (map.cc:406)
#define TR_TINY 2.2250738585072014e-308   // std::numeric_limits<double>::min(): makeHouseholder's threshold on the tail's squared norm

enum { TR_NONE = -1, TR_OK = 0, TR_FEW = 1, TR_RANK = 2, TR_BAD = 3 };


// cam = fx, fy, cx, cy -> cami = fxi, fyi, cx, cy; false when fx or fy is zero or not finite
AIRFE_HD bool tr_cam(const double* cam, double* cami) {
  if (!is_finite(cam[0]) || !is_finite(cam[1]) || cam[0] == 0.0 || cam[1] == 0.0) return false;
  cami[0] = 1.0 / cam[0]; cami[1] = 1.0 / cam[1]; cami[2] = cam[2]; cami[3] = cam[3];
  return true;
}

struct TrAcc {
  double M[9], g[3], C[3];
  int bad;
};

AIRFE_HD void tr_acc_init(TrAcc* a) {
#pragma unroll
  for (int k = 0; k < 9; ++k) a->M[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) a->g[k] = a->C[k] = 0.0;
  a->bad = 0;
}

// one observer: keypoint (x, y) of a frame whose stored pose is T (Twc, row-major 4 x 4; row 3 is not read)
AIRFE_HD void tr_acc_add(TrAcc* a, const double* cami, float x, float y, const double* T) {
  const double b0 = ((double)x - cami[2]) * cami[0], b1 = ((double)y - cami[3]) * cami[1], b2 = 1.0;
  double v[3], c[3], w[3];
  bool ok = is_finite((double)x) && is_finite((double)y);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    ok = ok && is_finite(T[4 * r]) && is_finite(T[4 * r + 1]) && is_finite(T[4 * r + 2]) && is_finite(T[4 * r + 3]);
    v[r] = (T[4 * r] * b0 + T[4 * r + 1] * b1) + T[4 * r + 2] * b2;
    c[r] = T[4 * r + 3];
  }
  const double s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  ok = ok && is_finite(s) && s != 0.0;
  const double inv = 1.0 / s;
  const double d = (v[0] * c[0] + v[1] * c[1]) + v[2] * c[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = v[r] * inv;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int q = 0; q < 3; ++q) a->M[3 * r + q] += w[r] * v[q];
    a->g[r] += w[r] * d;
    a->C[r] += c[r];
  }
  if (!ok) a->bad = 1;
}

// A (row-major 3 x 3), rhs -> the rank by the 1e-5 rule; x only with rank 3; rdiag [3] = R's diagonal (or nullptr).  Every index below is a constant:
// the arrays live in registers on the device.
AIRFE_HD int tr_qr_solve(const double* A, const double* rhs, double* x, double* rdiag) {
  double a[9], c[3];
  int perm[3] = {0, 1, 2};
#pragma unroll
  for (int k = 0; k < 9; ++k) a[k] = A[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = rhs[k];
  // ---- step 0: rows 0 .. 2, columns 0 .. 2
  {
    const double n0 = (a[0] * a[0] + a[3] * a[3]) + a[6] * a[6], n1 = (a[1] * a[1] + a[4] * a[4]) + a[7] * a[7], n2 = (a[2] * a[2] + a[5] * a[5]) + a[8] * a[8];
    int p = 0;
    double best = n0;
    if (n1 > best) { p = 1; best = n1; }
    if (n2 > best) p = 2;
    if (p == 1) {
      double t;
      t = a[0]; a[0] = a[1]; a[1] = t; t = a[3]; a[3] = a[4]; a[4] = t; t = a[6]; a[6] = a[7]; a[7] = t;
      perm[0] = 1; perm[1] = 0;
    } else if (p == 2) {
      double t;
      t = a[0]; a[0] = a[2]; a[2] = t; t = a[3]; a[3] = a[5]; a[5] = t; t = a[6]; a[6] = a[8]; a[8] = t;
      perm[0] = 2; perm[2] = 0;
    }
    const double tail = a[3] * a[3] + a[6] * a[6], c0 = a[0];
    double tau = 0.0, beta = c0, e1 = 0.0, e2 = 0.0;
    if (!(tail <= TR_TINY)) {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0.0) beta = -beta;
      e1 = a[3] / (c0 - beta);
      e2 = a[6] / (c0 - beta);
      tau = (beta - c0) / beta;
    }
    a[0] = beta;
    if (tau != 0.0) {
      const double t1 = tau * e1, t2 = tau * e2;
#pragma unroll
      for (int j = 1; j < 3; ++j) {
        double tmp = e1 * a[3 + j] + e2 * a[6 + j];
        tmp += a[j];
        a[j] -= tau * tmp;
        a[3 + j] -= t1 * tmp;
        a[6 + j] -= t2 * tmp;
      }
      double tmp = e1 * c[1] + e2 * c[2];
      tmp += c[0];
      c[0] -= tau * tmp;
      c[1] -= t1 * tmp;
      c[2] -= t2 * tmp;
    }
  }
  // ---- step 1: rows 1 .. 2, columns 1 .. 2
  {
    const double n1 = a[4] * a[4] + a[7] * a[7], n2 = a[5] * a[5] + a[8] * a[8];
    if (n2 > n1) {
      double t;
      t = a[1]; a[1] = a[2]; a[2] = t; t = a[4]; a[4] = a[5]; a[5] = t; t = a[7]; a[7] = a[8]; a[8] = t;
      const int q = perm[1]; perm[1] = perm[2]; perm[2] = q;
    }
    const double tail = a[7] * a[7], c0 = a[4];
    double tau = 0.0, beta = c0, e = 0.0;
    if (!(tail <= TR_TINY)) {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0.0) beta = -beta;
      e = a[7] / (c0 - beta);
      tau = (beta - c0) / beta;
    }
    a[4] = beta;
    if (tau != 0.0) {
      const double t1 = tau * e;
      double tmp = e * a[8];
      tmp += a[5];
      a[5] -= tau * tmp;
      a[8] -= t1 * tmp;
      tmp = e * c[2];
      tmp += c[1];
      c[1] -= tau * tmp;
      c[2] -= t1 * tmp;
    }
  }
  // ---- step 2: one row left: tau = 0, beta = the entry
  const double r0 = fabs(a[0]), r1 = fabs(a[4]), r2 = fabs(a[8]);
  if (rdiag) { rdiag[0] = a[0]; rdiag[1] = a[4]; rdiag[2] = a[8]; }
  double maxp = r0;
  if (r1 > maxp) maxp = r1;
  if (r2 > maxp) maxp = r2;
  const double thr = maxp * TR_RANK_TOL;
  const int rank = (r0 > thr ? 1 : 0) + (r1 > thr ? 1 : 0) + (r2 > thr ? 1 : 0);
  if (rank < 3) return rank;
  const double y2 = c[2] / a[8];
  const double y1 = (c[1] - a[5] * y2) / a[4];
  const double y0 = (c[0] - (a[1] * y1 + a[2] * y2)) / a[0];
#pragma unroll
  for (int r = 0; r < 3; ++r) x[r] = perm[0] == r ? y0 : (perm[1] == r ? y1 : y2);
  return rank;
}

// the accumulators of nobs observers -> the status; xyz [3] = the point, or NaN
AIRFE_HD int tr_finish(const TrAcc* a, int nobs, int min_observers, double* xyz) {
  xyz[0] = xyz[1] = xyz[2] = quiet_nan();
  if (nobs <= 0) return TR_NONE;
  if (nobs < (min_observers > 2 ? min_observers : 2)) return TR_FEW;
  if (a->bad) return TR_BAD;
  double A[9], rhs[3], x[3] = {0.0, 0.0, 0.0};
  const double n = (double)nobs;
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      A[3 * r + q] = (r == q ? n : 0.0) - a->M[3 * r + q];
      ok = ok && is_finite(A[3 * r + q]);
    }
    rhs[r] = a->C[r] - a->g[r];
    ok = ok && is_finite(rhs[r]);
  }
  if (!ok) return TR_BAD;
  if (tr_qr_solve(A, rhs, x, nullptr) < 3) return TR_RANK;
  if (!(is_finite(x[0]) && is_finite(x[1]) && is_finite(x[2]))) return TR_BAD;
  xyz[0] = x[0]; xyz[1] = x[1]; xyz[2] = x[2];
  return TR_OK;
}

// info i32 [4]: points ok, points observed (status != -1), points of status 2, points of status 3
AIRFE_HD void tr_info_flags(int status, int* f) {
  f[0] = status == TR_OK; f[1] = status != TR_NONE; f[2] = status == TR_RANK; f[3] = status == TR_BAD;
}

// One point on the host: Twc [n][16], xy [n][2] in observer order.  cami: tr_cam's.
inline int triangulate_point_host(const double* cami, const double* Twc, const float* xy, int n, int min_observers, double* xyz) {
  TrAcc a;
  tr_acc_init(&a);
  for (int k = 0; k < n; ++k) tr_acc_add(&a, cami, xy[2 * k], xy[2 * k + 1], Twc + (size_t)16 * k);
  return tr_finish(&a, n, min_observers, xyz);
}

// The host statement over the whole table.  feat [>= size][cap][feat_dim] (x, y at columns 1, 2 of a row), n [size], pose [>= size][16], point_id
// [>= size][cap]; xyz [max_points][3], status / nobs [max_points], info [4]: every entry is written.
inline void triangulate_build_host(const float* feat, int feat_dim, const int* n, const double* pose, const int32_t* point_id, int size, int cap, int max_points,
                                   const double* cami, int min_observers, double* xyz, int32_t* status, int32_t* nobs, int32_t* info) {
  std::vector<TrAcc> acc((size_t)max_points);
  std::vector<int> ids((size_t)(cap > 0 ? cap : 1));
  for (int m = 0; m < max_points; ++m) {
    tr_acc_init(&acc[m]);
    nobs[m] = 0;
  }
  for (int f = 0; f < size; ++f) {                                  // ascending frame index = observer order
    const int nf = clamp_count(n[f], cap);
    for (int i = 0; i < cap; ++i) {
      int ig;
      ids[i] = cv_row_id(point_id + (size_t)f * cap, i, nf, max_points, &ig);
    }
    for (int i = 0; i < cap; ++i) {
      if (!cv_first_occurrence(ids.data(), i)) continue;
      const float* row = feat + ((size_t)f * cap + i) * feat_dim;
      tr_acc_add(&acc[ids[i]], cami, row[1], row[2], pose + (size_t)f * 16);
      ++nobs[ids[i]];
    }
  }
  info[0] = info[1] = info[2] = info[3] = 0;
  for (int m = 0; m < max_points; ++m) {
    status[m] = tr_finish(&acc[m], nobs[m], min_observers, xyz + (size_t)3 * m);
    int fl[4];
    tr_info_flags(status[m], fl);
    for (int k = 0; k < 4; ++k) info[k] += fl[k];
  }
}

#endif  // AIRFE_TRIANGULATE_CORE_H_
