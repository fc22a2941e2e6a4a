// F-matrix RANSAC behind MatchingPoints(..., outlier_rejection = true) (src/point_matcher.cc:95-104: cv::findFundamentalMat(points0, points1,
// cv::FM_RANSAC, 20, 0.99, inliers)): the per-sample arithmetic of the contract in include/airfe.h ("F-matrix RANSAC"), written once for the HIP
// kernels (kernels_fransac.hip) and the C++ stand-in of cv::findFundamentalMat (shim/stubs/mini_support.cpp).  tests/fransac_ref.py restates it in numpy.
// fp64 throughout; no FMA contraction, so that the three statements round the same way (transcendentals aside: acos / cos / cbrt / log).
#ifndef AIRFE_FRANSAC_CORE_H_
#define AIRFE_FRANSAC_CORE_H_

#include <stdint.h>
#include <math.h>

#include "core_common.h"
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define FR_SEED 0x2545F4914F6CDD1DULL
#define FR_MAX_ATTEMPTS 64     // draws of one sample before it is given up (no model from it)
#define FR_RANSAC_ITERS 1000   // maxIters of findFundamentalMat
#define FR_LMEDS_ITERS 300     // round(log(0.01) / log(1 - 0.55^7)) = 300 (tests/fransac_ref.py checks the number)
#define FR_MIN_RANSAC 15       // 9..14 matches: LMedS
#define FR_THRESH2 400.0f      // 20 px, squared

AIRFE_HD uint64_t fr_splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
// index of slot `slot` (0..6) of draw `attempt` of sample `s` among n matches
AIRFE_HD int fr_draw(int s, int attempt, int slot, int n) {
  const uint64_t h = fr_splitmix64(FR_SEED ^ (((uint64_t)s << 32) | ((uint64_t)attempt << 8) | (uint64_t)slot));
  return (int)(((h >> 32) * (uint64_t)n) >> 32);
}

// OpenCV's collinearity form: |dx2*dy1 - dy2*dx1| <= FLT_EPSILON * (|dx1| + |dy1| + |dx2| + |dy2|)
AIRFE_HD bool fr_collinear(double xi, double yi, double xj, double yj, double xk, double yk) {
  const double dx1 = xj - xi, dy1 = yj - yi, dx2 = xk - xi, dy2 = yk - yi;
  return fabs(dx2 * dy1 - dy2 * dx1) <= 1.1920928955078125e-07 * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
}

// Draws sample s: X[k] = (x0, y0, x1, y1) of its 7 matches (xy: [n][4], truncated coordinates).  false: every attempt was degenerate.
template <typename T>
AIRFE_HD bool fr_sample(const T* xy, int n, int s, double X[7][4]) {
  for (int att = 0; att < FR_MAX_ATTEMPTS; ++att) {
    int id[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) id[k] = fr_draw(s, att, k, n);
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
      for (int b = a + 1; b < 7; ++b) ok = ok && id[a] != id[b];
    if (!ok) continue;
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) X[k][c] = (double)xy[4 * id[k] + c];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = i + 1; j < 7; ++j)
#pragma unroll
        for (int k = j + 1; k < 7; ++k)
          ok = ok && !fr_collinear(X[i][0], X[i][1], X[j][0], X[j][1], X[k][0], X[k][1]) &&
               !fr_collinear(X[i][2], X[i][3], X[j][2], X[j][3], X[k][2], X[k][3]);
    if (ok) return true;
  }
  return false;
}

AIRFE_HD double fr_det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// det of the matrix whose column j is Y's where bit j of `mask` is set, X's otherwise
AIRFE_HD double fr_det3_mix(const double* X, const double* Y, int mask) {
  double m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = (mask >> (i % 3)) & 1 ? Y[i] : X[i];
  return fr_det3(m);
}

// The 7-point solver: F[r][9] (row-major, x1^T F x0 = 0) for its 1..3 real roots, in root order; returns the number of models (0: degenerate).
AIRFE_HD int fr_solve7(const double X[7][4], double F[3][9]) {
  double A[7][9];
  double mx = 0.0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double x0 = X[k][0], y0 = X[k][1], x1 = X[k][2], y1 = X[k][3];
    A[k][0] = x1 * x0; A[k][1] = x1 * y0; A[k][2] = x1; A[k][3] = y1 * x0; A[k][4] = y1 * y0; A[k][5] = y1; A[k][6] = x0; A[k][7] = y0; A[k][8] = 1.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) mx = fabs(A[k][c]) > mx ? fabs(A[k][c]) : mx;
  }
  const double tol = 1e-12 * mx;
  bool ok = true;
  // Gaussian elimination with partial pivoting (first largest |pivot| wins) over columns 0..6; a pivot <= tol: no model
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    int p = k;
    double best = fabs(A[k][k]);
#pragma unroll
    for (int r = k + 1; r < 7; ++r)
      if (fabs(A[r][k]) > best) { best = fabs(A[r][k]); p = r; }
#pragma unroll
    for (int r = k + 1; r < 7; ++r) {
      const bool sw = r == p;
#pragma unroll
      for (int c = k; c < 9; ++c) {
        const double t = A[k][c];
        A[k][c] = sw ? A[r][c] : t;
        A[r][c] = sw ? t : A[r][c];
      }
    }
    ok = ok && best > tol;
#pragma unroll
    for (int r = k + 1; r < 7; ++r) {
      const double f = A[r][k] / A[k][k];
#pragma unroll
      for (int c = k + 1; c < 9; ++c) A[r][c] = A[r][c] - f * A[k][c];
    }
  }
  if (!ok) return 0;
  // null space: v1 = (.., 1, 0), v2 = (.., 0, 1) by back substitution
  double f1[9], f2[9];
  f1[7] = 1.0; f1[8] = 0.0; f2[7] = 0.0; f2[8] = 1.0;
#pragma unroll
  for (int k = 6; k >= 0; --k) {
    double s1 = A[k][7] * f1[7] + A[k][8] * f1[8], s2 = A[k][7] * f2[7] + A[k][8] * f2[8];
#pragma unroll
    for (int c = k + 1; c < 7; ++c) { s1 = s1 + A[k][c] * f1[c]; s2 = s2 + A[k][c] * f2[c]; }
    f1[k] = -s1 / A[k][k];
    f2[k] = -s2 / A[k][k];
  }
  // det(a F1 + (1 - a) F2) = det(F2 + a D), D = F1 - F2: c3 a^3 + c2 a^2 + c1 a + c0
  double D[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) D[i] = f1[i] - f2[i];
  const double c0 = fr_det3(f2), c3 = fr_det3(D);
  const double c1 = fr_det3_mix(f2, D, 1) + fr_det3_mix(f2, D, 2) + fr_det3_mix(f2, D, 4);
  const double c2 = fr_det3_mix(D, f2, 1) + fr_det3_mix(D, f2, 2) + fr_det3_mix(D, f2, 4);
  double rt[3] = {0.0, 0.0, 0.0};
  int nr = 0;
  if (c3 == 0.0) {
    if (c2 == 0.0) {
      if (c1 != 0.0) { rt[0] = -c0 / c1; nr = 1; }
    } else {
      const double disc = c1 * c1 - 4.0 * c2 * c0;
      if (disc == 0.0) { rt[0] = -c1 / (2.0 * c2); nr = 1; }
      else if (disc > 0.0) { const double sq = sqrt(disc); rt[0] = (-c1 + sq) / (2.0 * c2); rt[1] = (-c1 - sq) / (2.0 * c2); nr = 2; }
    }
  } else {
    const double a2 = c2 / c3, a1 = c1 / c3, a0 = c0 / c3;
    const double Q = (a2 * a2 - 3.0 * a1) / 9.0, R = (2.0 * a2 * a2 * a2 - 9.0 * a2 * a1 + 27.0 * a0) / 54.0;
    const double Q3 = Q * Q * Q, d = Q3 - R * R;
    if (d >= 0.0) {
      if (Q3 == 0.0) { rt[0] = -a2 / 3.0; nr = 1; }
      else {
        double t = R / sqrt(Q3);
        t = t > 1.0 ? 1.0 : (t < -1.0 ? -1.0 : t);
        const double th = acos(t), sq = -2.0 * sqrt(Q);
        rt[0] = sq * cos(th / 3.0) - a2 / 3.0;
        rt[1] = sq * cos((th + 6.283185307179586) / 3.0) - a2 / 3.0;
        rt[2] = sq * cos((th + 12.566370614359172) / 3.0) - a2 / 3.0;
        nr = 3;
      }
    } else if (d == d) {
      double e = cbrt(sqrt(-d) + fabs(R));
      if (R > 0.0) e = -e;
      rt[0] = e + Q / e - a2 / 3.0;
      nr = 1;
    }
  }
  int m = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (r >= nr) break;
    const double a = rt[r], b = 1.0 - a;
    double G[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] = a * f1[i] + b * f2[i];
    if (fabs(G[8]) > 2.220446049250313e-16) {       // OpenCV's scaling: F(2,2) = 1 where it is not ~0
      const double s = G[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) G[i] = G[i] / s;
      G[8] = 1.0;
    }
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && isfinite(G[i]);
    if (!fin) continue;
#pragma unroll
    for (int i = 0; i < 9; ++i) F[m][i] = G[i];
    ++m;
  }
  return m;
}

// the larger of the two squared point-to-epipolar-line distances, in double, rounded to float; NaN counts as +inf
AIRFE_HD float fr_error(const double* f, double x0, double y0, double x1, double y1) {
  const double a = f[0] * x0 + f[1] * y0 + f[2], b = f[3] * x0 + f[4] * y0 + f[5], c = f[6] * x0 + f[7] * y0 + f[8];
  const double d = x1 * a + y1 * b + c;
  const double ap = f[0] * x1 + f[3] * y1 + f[6], bp = f[1] * x1 + f[4] * y1 + f[7];
  double e1 = d * d / (ap * ap + bp * bp), e2 = d * d / (a * a + b * b);
  if (!(e1 >= 0.0)) e1 = INFINITY;
  if (!(e2 >= 0.0)) e2 = INFINITY;
  return (float)(e1 > e2 ? e1 : e2);
}

// RANSACUpdateNumIters(0.99, (n - good) / n, 7, 1000), with (1 - ep)^7 as repeated products
AIRFE_HD int fr_update_niters(int n, int good) {
  const double ep = (double)(n - good) / (double)n;
  const double num = 1.0 - 0.99;
  const double q = 1.0 - ep, q2 = q * q, q4 = q2 * q2;
  const double den = 1.0 - q4 * q2 * q;
  if (den < 2.2250738585072014e-308) return 0;
  const double ln = log(num), ld = log(den);
  return (ld >= 0.0 || -ln >= 1000.0 * (-ld)) ? FR_RANSAC_ITERS : (int)rint(ln / ld);
}

// LMedS inlier bound from the smallest median: sigma = max(2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median), 0.001); err <= (float)sigma^2
AIRFE_HD float fr_lmeds_thresh(int n, float median) {
  double sigma = 2.5 * 1.4826 * (1.0 + 5.0 / (double)(n - 7)) * sqrt((double)median);
  sigma = sigma > 0.001 ? sigma : 0.001;
  return (float)(sigma * sigma);
}

#endif  // AIRFE_FRANSAC_CORE_H_
