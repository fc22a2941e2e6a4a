// PnP RANSAC of SolvePnPWithCV (src/g2o_optimization/g2o_optimization.cc:1085-1134: cv::solvePnPRansac(object_points, image_points, K, 0, rvec, tvec,
// false, 100, 20.0, 0.99, inliers)) and the stereo back-projection that feeds it (src/frame.cc:141-172, src/camera.cc:275-280): the per-sample and
// per-problem arithmetic of the contract in include/airfe.h ("PnP RANSAC", "Stereo points"), written once for the HIP kernels (kernels_pnp.hip) and the
// host core (pnp_solve_host below).  tests/pnp_ref.py restates it in numpy.  fp64 throughout (the projections of the inlier test are rounded to float);
// no FMA contraction; the only non-rational operation is sqrt (correctly rounded on both sides), so host and device agree bit for bit.
// Every array lives behind a pointer: the kernels point it at LDS, so no per-lane array is indexed with a runtime value (no scratch).
#ifndef AIRFE_PNP_CORE_H_
#define AIRFE_PNP_CORE_H_

#include "fransac_core.h"   // fr_splitmix64, AIRFE_HD

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define PNP_SEED 0x6A09E667F3BCC909ULL
#define PNP_MAX_ATTEMPTS 64
#define PNP_MAX_ITERS 100       // iterationsCount of SolvePnPWithCV
#define PNP_MIN_POINTS 8        // g2o_optimization.cc:1108
#define PNP_MAX_POINTS 1024
#define PNP_THRESH2 400.0f      // reprojectionError 20 px, squared
#define PNP_JACOBI_SWEEPS 30
#define PNP_GN_ITERS 5
#define PNP_LM_ITERS 20
#define PNP_LM_LANES 64         // partial sums of the refinement: lane l takes the points l, l + 64, ...
#define PNP_PINV_TOL 1e-10      // a principal axis shorter than this times the longest one gets barycentric weight 0

// workspace of one sample (doubles)
#define PW_PW 0      // [5][3] object points
#define PW_UV 15     // [5][2] image points
#define PW_CW 25     // [4][3] control points
#define PW_AL 37     // [5][4] barycentric alphas
#define PW_MM 57     // [12][12] M^T M, diagonalised in place
#define PW_VV 201    // [12][12] its eigenvectors (columns)
#define PW_S3 345    // [3][3] / [4][4] small symmetric matrix
#define PW_V3 361    // [3][3] / [4][4] its eigenvectors
#define PW_L 377     // [6][10]
#define PW_RHO 437   // [6]
#define PW_NS 443    // [4][12] null vectors, smallest eigenvalue first
#define PW_BETA 491  // [4]
#define PW_CCS 495   // [4][3]
#define PW_PCS 507   // [5][3]
#define PW_SOL 522   // [12] R (row-major), t of the current solution
#define PW_BEST 534  // [12] the model
#define PW_LS 546    // [6][5] least-squares matrix, [5][6] augmented normal equations, [5] x, [6] Gauss-Newton rhs
#define PW_ROW 617   // [24] two rows of M
#define PW_C0 641    // [6] scratch: axis scales / centroids
#define PW_SS 647    // [9] cross-covariance of the alignment
#define PNP_WS 656

AIRFE_HD int pnp_draw(int s, int attempt, int slot, int n) {
  const uint64_t h = fr_splitmix64(PNP_SEED ^ (((uint64_t)s << 32) | ((uint64_t)attempt << 8) | (uint64_t)slot));
  return (int)(((h >> 32) * (uint64_t)n) >> 32);
}
// sample s: id[0..4] = five distinct indices of n; false after 64 attempts with a repeat
AIRFE_HD bool pnp_sample(int n, int s, int* id) {
  for (int att = 0; att < PNP_MAX_ATTEMPTS; ++att) {
    bool ok = true;
    for (int k = 0; k < 5; ++k) {
      id[k] = pnp_draw(s, att, k, n);
      for (int j = 0; j < k; ++j) ok = ok && id[j] != id[k];
    }
    if (ok) return true;
  }
  return false;
}

// ---- cyclic Jacobi on a symmetric n x n matrix A (row-major, both triangles), eigenvectors in the columns of V --------------------------------
AIRFE_HD void pnp_jacobi_cs(double app, double aqq, double apq, double* c, double* s, double* t) {
  const double th = (aqq - app) / (2.0 * apq);
  const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
  *c = 1.0 / sqrt(tt * tt + 1.0);
  *s = tt * *c;
  *t = tt;
}
// the part of rotation (p, q) that row k owns: no row reads what another row writes, so rows may run in any order (or in parallel)
AIRFE_HD void pnp_jacobi_row(double* A, double* V, int n, int k, int p, int q, double c, double s, double t, double apq) {
  if (k == p) {
    A[p * n + p] = A[p * n + p] - t * apq;
    A[p * n + q] = 0.0;
  } else if (k == q) {
    A[q * n + q] = A[q * n + q] + t * apq;
    A[q * n + p] = 0.0;
  } else {
    const double akp = A[k * n + p], akq = A[k * n + q];
    const double nkp = c * akp - s * akq, nkq = s * akp + c * akq;
    A[k * n + p] = nkp; A[p * n + k] = nkp;
    A[k * n + q] = nkq; A[q * n + k] = nkq;
  }
  const double vkp = V[k * n + p], vkq = V[k * n + q];
  V[k * n + p] = c * vkp - s * vkq;
  V[k * n + q] = s * vkp + c * vkq;
}
// stopping rule, checked before each sweep: sum of squared off-diagonal entries (p < q, row-major order) <= 1e-30 * sum of squared diagonal entries
AIRFE_HD bool pnp_jacobi_converged(const double* A, int n) {
  double off = 0.0, dia = 0.0;
  for (int p = 0; p < n; ++p) {
    dia = dia + A[p * n + p] * A[p * n + p];
    for (int q = p + 1; q < n; ++q) off = off + A[p * n + q] * A[p * n + q];
  }
  return off <= 1e-30 * dia;
}
AIRFE_HD void pnp_jacobi(double* A, double* V, int n) {
  for (int i = 0; i < n * n; ++i) V[i] = (i % (n + 1)) == 0 ? 1.0 : 0.0;
  for (int sw = 0; sw < PNP_JACOBI_SWEEPS; ++sw) {
    if (pnp_jacobi_converged(A, n)) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        double c, s, t;
        pnp_jacobi_cs(A[p * n + p], A[q * n + q], apq, &c, &s, &t);
        for (int k = 0; k < n; ++k) pnp_jacobi_row(A, V, n, k, p, q, c, s, t, apq);
      }
  }
}
// rank r (0 = smallest) of eigenvalue i among the diagonal of A: ties go to the lower index
AIRFE_HD int pnp_rank(const double* A, int n, int i) {
  int r = 0;
  const double di = A[i * n + i];
  for (int j = 0; j < n; ++j) {
    const double dj = A[j * n + j];
    r += (dj < di || (dj == di && j < i)) ? 1 : 0;
  }
  return r;
}

// ---- least squares: the rows x cols matrix A (row-major, stride cols) and rhs b through the normal equations, Gaussian elimination with partial
// pivoting (first largest |pivot|); a pivot that is not > 0 in magnitude: false
AIRFE_HD bool pnp_gauss(double* N, int m, double* x) {   // N: [m][m + 1] augmented
  for (int k = 0; k < m; ++k) {
    int p = k;
    double best = fabs(N[k * (m + 1) + k]);
    for (int r = k + 1; r < m; ++r)
      if (fabs(N[r * (m + 1) + k]) > best) { best = fabs(N[r * (m + 1) + k]); p = r; }
    if (!(best > 0.0)) return false;
    if (p != k)
      for (int c = k; c <= m; ++c) { const double tmp = N[k * (m + 1) + c]; N[k * (m + 1) + c] = N[p * (m + 1) + c]; N[p * (m + 1) + c] = tmp; }
    for (int r = k + 1; r < m; ++r) {
      const double f = N[r * (m + 1) + k] / N[k * (m + 1) + k];
      for (int c = k; c <= m; ++c) N[r * (m + 1) + c] = N[r * (m + 1) + c] - f * N[k * (m + 1) + c];
    }
  }
  for (int k = m - 1; k >= 0; --k) {
    double s = N[k * (m + 1) + m];
    for (int c = k + 1; c < m; ++c) s = s - N[k * (m + 1) + c] * x[c];
    x[k] = s / N[k * (m + 1) + k];
  }
  return true;
}
AIRFE_HD bool pnp_lsq(const double* A, const double* b, int rows, int cols, double* N, double* x) {
  for (int r = 0; r < cols; ++r) {
    for (int c = 0; c < cols; ++c) {
      double s = 0.0;
      for (int i = 0; i < rows; ++i) s = s + A[i * cols + r] * A[i * cols + c];
      N[r * (cols + 1) + c] = s;
    }
    double s = 0.0;
    for (int i = 0; i < rows; ++i) s = s + A[i * cols + r] * b[i];
    N[r * (cols + 1) + cols] = s;
  }
  return pnp_gauss(N, cols, x);
}

// ---- projection ------------------------------------------------------------------------------------------------------------------------------
// Xc = R X + t in double, 1/z (1 where z == 0, as cvProjectPoints2), u = x / z * fx + cx
AIRFE_HD void pnp_project(const double* Rt, double X, double Y, double Z, const double* K, double* u, double* v) {
  const double xc = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[9];
  const double yc = Rt[3] * X + Rt[4] * Y + Rt[5] * Z + Rt[10];
  const double zc = Rt[6] * X + Rt[7] * Y + Rt[8] * Z + Rt[11];
  const double iz = zc != 0.0 ? 1.0 / zc : 1.0;
  *u = xc * iz * K[0] + K[2];
  *v = yc * iz * K[1] + K[3];
}
// the inlier test's error: the projection rounded to float, err = dx^2 + dy^2 in float
AIRFE_HD float pnp_error(const double* Rt, float X, float Y, float Z, float u, float v, const double* K) {
  double pu, pv;
  pnp_project(Rt, (double)X, (double)Y, (double)Z, K, &pu, &pv);
  const float dx = u - (float)pu, dy = v - (float)pv;
  return dx * dx + dy * dy;
}

// ---- EPnP on the five points in ws[PW_PW], ws[PW_UV] -----------------------------------------------------------------------------------------
// rows a, b of control-point pair j (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
AIRFE_HD int pnp_pair_a(int j) { return j < 3 ? 0 : (j < 5 ? 1 : 2); }
AIRFE_HD int pnp_pair_b(int j) { return j < 3 ? j + 1 : (j < 5 ? j - 1 : 3); }


// R, t of ws[PW_SOL] from ws[PW_BETA]: control points in the camera frame (sign: z of the first point >= 0), Horn's quaternion alignment of the
// object points onto them.  Returns the summed reprojection distance over the five points (NaN when anything is not finite).
AIRFE_HD double pnp_compute_rt(double* ws, const double* K) {
  double* ccs = ws + PW_CCS;
  double* pcs = ws + PW_PCS;
  const double* pw = ws + PW_PW;
  for (int j = 0; j < 12; ++j) ccs[j] = 0.0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 12; ++j) ccs[j] = ccs[j] + ws[PW_BETA + i] * ws[PW_NS + 12 * i + j];
  for (int i = 0; i < 5; ++i)
    for (int c = 0; c < 3; ++c) {
      const double* a = ws + PW_AL + 4 * i;
      pcs[3 * i + c] = a[0] * ccs[c] + a[1] * ccs[3 + c] + a[2] * ccs[6 + c] + a[3] * ccs[9 + c];
    }
  if (pcs[2] < 0.0) {
    for (int j = 0; j < 12; ++j) ccs[j] = -ccs[j];
    for (int j = 0; j < 15; ++j) pcs[j] = -pcs[j];
  }
  double* c0 = ws + PW_C0;    // pc0 [3], pw0 [3]
  for (int c = 0; c < 3; ++c) {
    double sc = 0.0, sw = 0.0;
    for (int i = 0; i < 5; ++i) { sc = sc + pcs[3 * i + c]; sw = sw + pw[3 * i + c]; }
    c0[c] = sc / 5.0; c0[3 + c] = sw / 5.0;
  }
  double* S = ws + PW_SS;     // S[a][b] = sum (pw - pw0)_a (pc - pc0)_b
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
      for (int i = 0; i < 5; ++i) s = s + (pw[3 * i + a] - c0[3 + a]) * (pcs[3 * i + b] - c0[b]);
      S[3 * a + b] = s;
    }
  double* N = ws + PW_S3;
  double* V = ws + PW_V3;
  N[0] = (S[0] + S[4]) + S[8];  N[1] = S[5] - S[7];          N[2] = S[6] - S[2];          N[3] = S[1] - S[3];
  N[5] = (S[0] - S[4]) - S[8];  N[6] = S[1] + S[3];          N[7] = S[6] + S[2];
  N[10] = (S[4] - S[0]) - S[8]; N[11] = S[5] + S[7];
  N[15] = (S[8] - S[0]) - S[4];
  N[4] = N[1]; N[8] = N[2]; N[12] = N[3]; N[9] = N[6]; N[13] = N[7]; N[14] = N[11];
  pnp_jacobi(N, V, 4);
  int col = 0;
  for (int j = 0; j < 4; ++j) col = pnp_rank(N, 4, j) == 3 ? j : col;
  double w = V[col], x = V[4 + col], y = V[8 + col], z = V[12 + col];
  const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm;
  double* R = ws + PW_SOL;
  const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
  R[0] = ((ww + xx) - yy) - zz;  R[1] = 2.0 * (x * y - w * z);  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);  R[4] = ((ww - xx) + yy) - zz;  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);  R[7] = 2.0 * (y * z + w * x);  R[8] = ((ww - xx) - yy) + zz;
  for (int r = 0; r < 3; ++r) R[9 + r] = c0[r] - ((R[3 * r] * c0[3] + R[3 * r + 1] * c0[4]) + R[3 * r + 2] * c0[5]);
  double err = 0.0;
  for (int i = 0; i < 5; ++i) {
    double u, v;
    pnp_project(R, pw[3 * i], pw[3 * i + 1], pw[3 * i + 2], K, &u, &v);
    const double du = u - ws[PW_UV + 2 * i], dv = v - ws[PW_UV + 2 * i + 1];
    err = err + sqrt(du * du + dv * dv);
  }
  bool fin = isfinite(err);
  for (int j = 0; j < 12; ++j) fin = fin && isfinite(R[j]);
  return fin ? err : NAN;
}

// EPnP (Lepetit, Moreno-Noguer & Fua 2009) on the five points of ws[PW_PW] / ws[PW_UV]; the model (R row-major, t) in ws[PW_BEST]; false: no model
AIRFE_HD bool pnp_epnp(double* ws, const double* K) {
  const double* pw = ws + PW_PW;
  double* cw = ws + PW_CW;
  double* al = ws + PW_AL;
  // control points: the centroid, then the centroid + sqrt(lambda_j / 5) u_j along the principal axes, largest eigenvalue first
  for (int c = 0; c < 3; ++c) {
    double s = 0.0;
    for (int i = 0; i < 5; ++i) s = s + pw[3 * i + c];
    cw[c] = s / 5.0;
  }
  double* S3 = ws + PW_S3;
  double* V3 = ws + PW_V3;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
      for (int i = 0; i < 5; ++i) s = s + (pw[3 * i + a] - cw[a]) * (pw[3 * i + b] - cw[b]);
      S3[3 * a + b] = s;
    }
  pnp_jacobi(S3, V3, 3);
  double* sc = ws + PW_C0;    // scale of axis j [3], its eigenvector column [3]
  for (int col = 0; col < 3; ++col) {
    const int j = 2 - pnp_rank(S3, 3, col);
    const double d = S3[4 * col];
    sc[j] = sqrt((d > 0.0 ? d : 0.0) / 5.0);
    sc[3 + j] = (double)col;
  }
  for (int j = 0; j < 3; ++j) {
    const int col = (int)sc[3 + j];
    for (int c = 0; c < 3; ++c) cw[3 * (j + 1) + c] = cw[c] + sc[j] * V3[3 * c + col];
  }
  // barycentric alphas through the pseudo-inverse of [s_j u_j]: alpha_j = u_j . (p - c0) / s_j, 0 where s_j <= 1e-10 s_0
  for (int i = 0; i < 5; ++i) {
    for (int j = 0; j < 3; ++j) {
      const int col = (int)sc[3 + j];
      const double proj = (pw[3 * i] - cw[0]) * V3[col] + (pw[3 * i + 1] - cw[1]) * V3[3 + col] + (pw[3 * i + 2] - cw[2]) * V3[6 + col];
      al[4 * i + 1 + j] = sc[j] > PNP_PINV_TOL * sc[0] ? proj / sc[j] : 0.0;
    }
    al[4 * i] = ((1.0 - al[4 * i + 1]) - al[4 * i + 2]) - al[4 * i + 3];
  }
  // M^T M over the two rows of every point: [a_j fx, 0, a_j (cx - u)], [0, a_j fy, a_j (cy - v)]
  double* MM = ws + PW_MM;
  double* row = ws + PW_ROW;
  for (int j = 0; j < 144; ++j) MM[j] = 0.0;
  for (int i = 0; i < 5; ++i) {
    const double u = ws[PW_UV + 2 * i], v = ws[PW_UV + 2 * i + 1];
    for (int j = 0; j < 4; ++j) {
      const double a = al[4 * i + j];
      row[3 * j] = a * K[0]; row[3 * j + 1] = 0.0; row[3 * j + 2] = a * (K[2] - u);
      row[12 + 3 * j] = 0.0; row[12 + 3 * j + 1] = a * K[1]; row[12 + 3 * j + 2] = a * (K[3] - v);
    }
    for (int r = 0; r < 12; ++r)
      for (int c = r; c < 12; ++c) MM[12 * r + c] = MM[12 * r + c] + (row[r] * row[c] + row[12 + r] * row[12 + c]);
  }
  for (int r = 1; r < 12; ++r)
    for (int c = 0; c < r; ++c) MM[12 * r + c] = MM[12 * c + r];
  pnp_jacobi(MM, ws + PW_VV, 12);
  for (int j = 0; j < 48; ++j) ws[PW_NS + j] = 0.0;             // (NaN eigenvalues can leave a rank unfilled)
  for (int col = 0; col < 12; ++col) {
    const int r = pnp_rank(MM, 12, col);
    if (r < 4)
      for (int j = 0; j < 12; ++j) ws[PW_NS + 12 * r + j] = ws[PW_VV + 12 * j + col];
  }
  // L_6x10 and rho over the control-point pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
  double* L = ws + PW_L;
  double* dv = row;           // dv[k][c] = v_k[a] - v_k[b]
  for (int i = 0; i < 6; ++i) {
    const int a = pnp_pair_a(i), b = pnp_pair_b(i);
    for (int k = 0; k < 4; ++k)
      for (int c = 0; c < 3; ++c) dv[3 * k + c] = ws[PW_NS + 12 * k + 3 * a + c] - ws[PW_NS + 12 * k + 3 * b + c];
#define PNP_DOT(k, l) (dv[3 * (k)] * dv[3 * (l)] + dv[3 * (k) + 1] * dv[3 * (l) + 1] + dv[3 * (k) + 2] * dv[3 * (l) + 2])
    double* l = L + 10 * i;
    l[0] = PNP_DOT(0, 0); l[1] = 2.0 * PNP_DOT(0, 1); l[2] = PNP_DOT(1, 1); l[3] = 2.0 * PNP_DOT(0, 2); l[4] = 2.0 * PNP_DOT(1, 2);
    l[5] = PNP_DOT(2, 2); l[6] = 2.0 * PNP_DOT(0, 3); l[7] = 2.0 * PNP_DOT(1, 3); l[8] = 2.0 * PNP_DOT(2, 3); l[9] = PNP_DOT(3, 3);
#undef PNP_DOT
    const double d0 = cw[3 * a] - cw[3 * b], d1 = cw[3 * a + 1] - cw[3 * b + 1], d2 = cw[3 * a + 2] - cw[3 * b + 2];
    ws[PW_RHO + i] = d0 * d0 + d1 * d1 + d2 * d2;
  }
  // betas for N = 1, 2, 3, each refined by Gauss-Newton; the solution with the smallest reprojection distance wins (the first on ties)
  double* A = ws + PW_LS;
  double* NE = ws + PW_LS + 30;
  double* x = ws + PW_LS + 60;
  double* res = ws + PW_LS + 65;
  double* be = ws + PW_BETA;
  double best = INFINITY;
  bool found = false;
  for (int N = 1; N <= 3; ++N) {
    const int cols = N == 1 ? 4 : (N == 2 ? 3 : 5);
    for (int i = 0; i < 6; ++i)
      for (int c = 0; c < cols; ++c) A[cols * i + c] = L[10 * i + (N == 1 ? (c == 0 ? 0 : (c == 1 ? 1 : (c == 2 ? 3 : 6))) : c)];
    if (!pnp_lsq(A, ws + PW_RHO, 6, cols, NE, x)) continue;
    if (N == 1) {
      const double s = x[0] < 0.0 ? sqrt(-x[0]) : sqrt(x[0]);
      const double sg = x[0] < 0.0 ? -1.0 : 1.0;
      be[0] = s; be[1] = sg * x[1] / s; be[2] = sg * x[2] / s; be[3] = sg * x[3] / s;
    } else {
      const double x2 = x[2];
      if (x[0] < 0.0) { be[0] = sqrt(-x[0]); be[1] = x2 < 0.0 ? sqrt(-x2) : 0.0; }
      else { be[0] = sqrt(x[0]); be[1] = x2 > 0.0 ? sqrt(x2) : 0.0; }
      if (x[1] < 0.0) be[0] = -be[0];
      be[2] = N == 3 ? x[3] / be[0] : 0.0;
      be[3] = 0.0;
    }
    for (int it = 0; it < PNP_GN_ITERS; ++it) {
      for (int i = 0; i < 6; ++i) {
        const double* l = L + 10 * i;
        const double b0 = be[0], b1 = be[1], b2 = be[2], b3 = be[3];
        A[4 * i + 0] = 2.0 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3;
        A[4 * i + 1] = l[1] * b0 + 2.0 * l[2] * b1 + l[4] * b2 + l[7] * b3;
        A[4 * i + 2] = l[3] * b0 + l[4] * b1 + 2.0 * l[5] * b2 + l[8] * b3;
        A[4 * i + 3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2.0 * l[9] * b3;
        res[i] = ws[PW_RHO + i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2 + l[5] * b2 * b2 +
                                   l[6] * b0 * b3 + l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3);
      }
      if (!pnp_lsq(A, res, 6, 4, NE, x)) break;
      for (int k = 0; k < 4; ++k) be[k] = be[k] + x[k];
    }
    const double err = pnp_compute_rt(ws, K);
    if (err == err && (!found || err < best)) {
      found = true;
      best = err;
      for (int j = 0; j < 12; ++j) ws[PW_BEST + j] = ws[PW_SOL + j];
    }
  }
  return found;
}

// sample s of a problem of n points: draw, gather, solve.  id [5] ints; ws [PNP_WS].  false: no model
AIRFE_HD bool pnp_solve_sample(const float* obj, const float* img, int n, int s, const double* K, int* id, double* ws) {
  if (!pnp_sample(n, s, id)) return false;
  for (int k = 0; k < 5; ++k) {
    const int i = id[k];
    ws[PW_PW + 3 * k] = (double)obj[3 * i]; ws[PW_PW + 3 * k + 1] = (double)obj[3 * i + 1]; ws[PW_PW + 3 * k + 2] = (double)obj[3 * i + 2];
    ws[PW_UV + 2 * k] = (double)img[2 * i]; ws[PW_UV + 2 * k + 1] = (double)img[2 * i + 1];
  }
  return pnp_epnp(ws, K);
}

// ---- the sequential rule ------------------------------------------------------------------------------------------------------------------------
// RANSACUpdateNumIters(0.99, (n - good) / n, 5, maxIters), (1 - ep)^5 as repeated products
AIRFE_HD int pnp_update_niters(int n, int good, int max_iters) {
  const double ep = (double)(n - good) / (double)n;
  const double num = 1.0 - 0.99;
  const double q = 1.0 - ep, q2 = q * q, q4 = q2 * q2;
  const double den = 1.0 - q4 * q;
  if (den < 2.2250738585072014e-308) return 0;
  const double ln = log(num), ld = log(den);
  return (ld >= 0.0 || -ln >= (double)max_iters * (-ld)) ? max_iters : (int)rint(ln / ld);
}
// scores [100]: inliers per sample (-1: no model).  The selected sample (-1: none); *best = its inlier count
AIRFE_HD int pnp_select(const int* scores, int n, int* best) {
  int niters = PNP_MAX_ITERS, bc = 0, win = -1;
  for (int s = 0; s < niters && s < PNP_MAX_ITERS; ++s) {
    const int c = scores[s];
    if (c > (bc > 4 ? bc : 4)) {
      bc = c; win = s;
      niters = pnp_update_niters(n, c, niters);
    }
  }
  *best = win < 0 ? 0 : bc;
  return win;
}

// ---- Levenberg-Marquardt refinement --------------------------------------------------------------------------------------------------------
// parameters: the update (w, tau) maps R, t to Cay(w) R, t + tau with Cay(w) = I + 2 / (1 + w.w) ([w]x + [w]x^2) (rational: no sqrt, no trig)
// per point: o[0..20] = J^T J (upper triangle, row-major), o[21..26] = J^T r, o[27] = r^T r; J [12] = the two rows of the Jacobian
AIRFE_HD void pnp_lm_point(const double* Rt, double X, double Y, double Z, double u, double v, const double* K, double* J, double* o) {
  const double p0 = Rt[0] * X + Rt[1] * Y + Rt[2] * Z, p1 = Rt[3] * X + Rt[4] * Y + Rt[5] * Z, p2 = Rt[6] * X + Rt[7] * Y + Rt[8] * Z;
  const double xc = p0 + Rt[9], yc = p1 + Rt[10], zc = p2 + Rt[11];
  if (zc == 0.0) {
    for (int k = 0; k < 28; ++k) o[k] = 0.0;
    return;
  }
  const double iz = 1.0 / zc, a = xc * iz, b = yc * iz;
  const double ru = (a * K[0] + K[2]) - u, rv = (b * K[1] + K[3]) - v;
  const double gu0 = K[0] * iz, gu2 = -(K[0] * a * iz), gv1 = K[1] * iz, gv2 = -(K[1] * b * iz);
  J[0] = gu2 * (2.0 * p1); J[1] = gu0 * (2.0 * p2) + gu2 * (-2.0 * p0); J[2] = gu0 * (-2.0 * p1); J[3] = gu0; J[4] = 0.0; J[5] = gu2;
  J[6] = gv1 * (-2.0 * p2) + gv2 * (2.0 * p1); J[7] = gv2 * (-2.0 * p0); J[8] = gv1 * (2.0 * p0); J[9] = 0.0; J[10] = gv1; J[11] = gv2;
  int m = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) o[m++] = J[r] * J[c] + J[6 + r] * J[6 + c];
  for (int r = 0; r < 6; ++r) o[21 + r] = J[r] * ru + J[6 + r] * rv;
  o[27] = ru * ru + rv * rv;
}

// state S [PL_SIZE]
#define PL_CUR 0     // [12] current R, t
#define PL_TRY 12    // [12] trial
#define PL_ACC 24    // [28] sums at the current pose
#define PL_LAM 52
#define PL_STOP 53
#define PL_DEL 54    // [6] the step
#define PL_AUG 60    // [6][7] damped normal equations, then Cay(w) [9]
#define PL_SIZE 102

AIRFE_HD void pnp_lm_start(double* S, const double* Rt, const double* tot) {
  for (int k = 0; k < 12; ++k) S[PL_CUR + k] = Rt[k];
  for (int k = 0; k < 28; ++k) S[PL_ACC + k] = tot[k];
  S[PL_LAM] = 1e-3;
  S[PL_STOP] = (isfinite(tot[27]) && tot[27] > 0.0) ? 0.0 : 1.0;
}
// Cay(w) = I + 2 / (1 + w.w) ([w]x + [w]x^2), row-major in C [9] (shared with poseopt_core.h)
AIRFE_HD void pnp_cayley(double w0, double w1, double w2, double* C) {
  const double nn = (w0 * w0 + w1 * w1) + w2 * w2, k = 2.0 / (1.0 + nn);
  C[0] = 1.0 + k * (w0 * w0 - nn); C[1] = k * (-w2 + w0 * w1);      C[2] = k * (w1 + w0 * w2);
  C[3] = k * (w2 + w1 * w0);       C[4] = 1.0 + k * (w1 * w1 - nn); C[5] = k * (-w0 + w1 * w2);
  C[6] = k * (-w1 + w2 * w0);      C[7] = k * (w0 + w2 * w1);       C[8] = 1.0 + k * (w2 * w2 - nn);
}
AIRFE_HD int pnp_uidx(int r, int c) { return r * 6 - (r * (r - 1)) / 2 + (c - r); }
// (A + lambda diag(A)) delta = -g; the trial pose.  A singular system stops the refinement.
AIRFE_HD void pnp_lm_propose(double* S) {
  double* N = S + PL_AUG;
  const double lam = S[PL_LAM];
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) {
      const double a = S[PL_ACC + (r <= c ? pnp_uidx(r, c) : pnp_uidx(c, r))];
      N[7 * r + c] = r == c ? a * (1.0 + lam) : a;
    }
    N[7 * r + 6] = -S[PL_ACC + 21 + r];
  }
  double* d = S + PL_DEL;
  if (!pnp_gauss(N, 6, d)) { S[PL_STOP] = 1.0; return; }
  double* C = N;
  pnp_cayley(d[0], d[1], d[2], C);
  const double* R = S + PL_CUR;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) S[PL_TRY + 3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
  for (int r = 0; r < 3; ++r) S[PL_TRY + 9 + r] = R[9 + r] + d[3 + r];
}
// a trial with a smaller cost is taken (lambda / 10; stop when max |delta| < FLT_EPSILON), otherwise lambda * 10
AIRFE_HD void pnp_lm_judge(double* S, const double* tot) {
  if (tot[27] < S[PL_ACC + 27]) {
    for (int k = 0; k < 12; ++k) S[PL_CUR + k] = S[PL_TRY + k];
    for (int k = 0; k < 28; ++k) S[PL_ACC + k] = tot[k];
    S[PL_LAM] = S[PL_LAM] / 10.0;
    double mx = 0.0;
    for (int k = 0; k < 6; ++k) mx = fabs(S[PL_DEL + k]) > mx ? fabs(S[PL_DEL + k]) : mx;
    if (mx < 1.1920928955078125e-07) S[PL_STOP] = 1.0;
  } else {
    S[PL_LAM] = S[PL_LAM] * 10.0;
  }
}
// Twc (16, row-major) of SolvePnPWithCV: Rwc = Rcw^T, twc = Rwc (-tcw)
AIRFE_HD void pnp_twc(const double* Rt, double* T) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[4 * r + c] = Rt[3 * c + r];
    T[4 * r + 3] = (Rt[r] * (-Rt[9]) + Rt[3 + r] * (-Rt[10])) + Rt[6 + r] * (-Rt[11]);
    T[12 + r] = 0.0;
  }
  T[15] = 1.0;
}
AIRFE_HD bool pnp_finite12(const double* Rt) {
  bool f = true;
  for (int k = 0; k < 12; ++k) f = f && isfinite(Rt[k]);
  return f;
}

// ---- stereo back-projection (Frame::AddRightFeatures, src/frame.cc:141-172; Camera::BackProjectStereo, src/camera.cc:275-280) ------------------
// cam [8] = min_x_diff, max_x_diff, max_y_diff, bf, fx, fy, cx, cy
AIRFE_HD bool pnp_stereo_good(float xl, float yl, float xr, float yr, const double* cam) {
  const double dx = (double)fabsf(xl - xr), dy = (double)fabsf(yl - yr);
  if (!(dx > cam[0] && dx < cam[1] && dy <= cam[2])) return false;
  const double par = (double)(xl - xr);
  return par < cam[1] && par > cam[0];
}
// o = u_right, depth (bf / the float parallax), X, Y, Z (bf / the double difference x - u_right)
AIRFE_HD void pnp_stereo_point(float xl, float yl, float xr, const double* cam, double* o) {
  const double par = (double)(xl - xr);
  o[0] = (double)xr;
  o[1] = cam[3] / par;
  const double x = ((double)xl - cam[6]) * (1.0 / cam[4]), y = ((double)yl - cam[7]) * (1.0 / cam[5]);
  const double d = cam[3] / ((double)xl - o[0]);
  o[2] = x * d; o[3] = y * d; o[4] = 1.0 * d;
}

// ---- the host core: the whole contract for one problem, serially (the kernels compute the same bits) ------------------------------------------
// obj [n][3], img [n][2] floats; K = fx, fy, cx, cy.  Outputs: Twc [16], Rt [12] (Rcw row-major, tcw; may be NULL), mask [n], *count; scores [100]
// (may be NULL): inliers per sample, -1 = no model.  Returns the selected sample (-1: none).
inline int pnp_solve_host(const float* obj, const float* img, int n, const double* K, double* Twc, double* Rt, uint8_t* mask, int* count,
                          int* scores_out) {
  static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  double ws[PNP_WS], models[PNP_MAX_ITERS * 12], part[PNP_LM_LANES * 28], tot[28], S[PL_SIZE], J[12], o[28];
  int scores[PNP_MAX_ITERS], id[5];
  for (int s = 0; s < PNP_MAX_ITERS; ++s) scores[s] = -1;
  for (int i = 0; i < n; ++i) mask[i] = 0;
  int win = -1, best = 0;
  if (n >= PNP_MIN_POINTS) {
    for (int s = 0; s < PNP_MAX_ITERS; ++s) {
      if (!pnp_solve_sample(obj, img, n, s, K, id, ws)) continue;
      for (int k = 0; k < 12; ++k) models[12 * s + k] = ws[PW_BEST + k];
      int c = 0;
      for (int i = 0; i < n; ++i) c += pnp_error(ws + PW_BEST, obj[3 * i], obj[3 * i + 1], obj[3 * i + 2], img[2 * i], img[2 * i + 1], K) <= PNP_THRESH2;
      scores[s] = c;
    }
    win = pnp_select(scores, n, &best);
  }
  if (scores_out)
    for (int s = 0; s < PNP_MAX_ITERS; ++s) scores_out[s] = scores[s];
  const double* res = I12;
  if (win >= 0) {
    const double* M = models + 12 * win;
    for (int i = 0; i < n; ++i) mask[i] = pnp_error(M, obj[3 * i], obj[3 * i + 1], obj[3 * i + 2], img[2 * i], img[2 * i + 1], K) <= PNP_THRESH2;
    auto accumulate = [&](const double* P) {
      for (int k = 0; k < PNP_LM_LANES * 28; ++k) part[k] = 0.0;
      for (int l = 0; l < PNP_LM_LANES; ++l)
        for (int i = l; i < n; i += PNP_LM_LANES) {
          if (!mask[i]) continue;
          pnp_lm_point(P, (double)obj[3 * i], (double)obj[3 * i + 1], (double)obj[3 * i + 2], (double)img[2 * i], (double)img[2 * i + 1], K, J, o);
          for (int k = 0; k < 28; ++k) part[28 * l + k] = part[28 * l + k] + o[k];
        }
      for (int k = 0; k < 28; ++k) {
        double t = 0.0;
        for (int l = 0; l < PNP_LM_LANES; ++l) t = t + part[28 * l + k];
        tot[k] = t;
      }
    };
    accumulate(M);
    pnp_lm_start(S, M, tot);
    for (int it = 0; it < PNP_LM_ITERS; ++it) {
      if (S[PL_STOP] != 0.0) break;
      pnp_lm_propose(S);
      if (S[PL_STOP] != 0.0) break;
      accumulate(S + PL_TRY);
      pnp_lm_judge(S, tot);
    }
    res = pnp_finite12(S + PL_CUR) ? S + PL_CUR : M;
  }
  if (win >= 0) {
    pnp_twc(res, Twc);
  } else {
    for (int k = 0; k < 16; ++k) Twc[k] = (k % 5) == 0 ? 1.0 : 0.0;
  }
  if (Rt)
    for (int k = 0; k < 12; ++k) Rt[k] = res[k];
  *count = win >= 0 ? best : 0;
  return win;
}

// Frame::AddRightFeatures + BackProjectPoint on host rows: fl [nl][259], fr [.][259], idx [m][2] (left, right; in range).  u_right / depth [nl] (-1 where
// unset), xyz [nl][3] (NaN where unset).  Returns the number of list entries that pass (= airfe_seq_good_stereo_points).
inline int pnp_stereo_host(const float* fl, int nl, const float* fr, const int32_t* idx, int m, const double* cam, double* u_right, double* depth,
                           double* xyz) {
  for (int i = 0; i < nl; ++i) { u_right[i] = -1.0; depth[i] = -1.0; xyz[3 * i] = xyz[3 * i + 1] = xyz[3 * i + 2] = NAN; }
  int good = 0;
  double o[5];
  for (int j = 0; j < m; ++j) {
    const float* a = fl + (size_t)idx[2 * j] * 259;
    const float* b = fr + (size_t)idx[2 * j + 1] * 259;
    if (!pnp_stereo_good(a[1], a[2], b[1], b[2], cam)) continue;
    ++good;
    pnp_stereo_point(a[1], a[2], b[1], cam, o);
    const int i = idx[2 * j];
    u_right[i] = o[0]; depth[i] = o[1]; xyz[3 * i] = o[2]; xyz[3 * i + 1] = o[3]; xyz[3 * i + 2] = o[4];
  }
  return good;
}

#endif  // AIRFE_PNP_CORE_H_
