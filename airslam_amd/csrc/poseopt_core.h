// Pose-only frame optimisation: the vision-only, points-only FrameOptimization call of tracking (src/map_builder.cc:353-417 ->
// src/g2o_optimization/g2o_optimization.cc:446-898 with one free VIPose, mono / stereo reprojection edges, Huber kernels, three rounds of optimize(10)
// and a chi-square classification after each).  The per-edge and per-problem arithmetic of the contract in include/airfe.h ("Frame optimisation"),
// written once for the HIP kernel (kernels_poseopt.hip) and the host core (poseopt_solve_host below).  tests/poseopt_ref.py restates it in Python.
// fp64 throughout (the chi2 of the classification is rounded to float); no FMA contraction; the only non-rational operation is sqrt, so host and device
// agree bit for bit.  The Gaussian elimination and the Cayley map are pnp_core.h's.  Every array that is indexed with a runtime value lives behind a
// pointer (the kernel points it at LDS); the per-edge accumulators are indexed with constants only, so the kernel keeps them in registers.
#ifndef AIRFE_POSEOPT_CORE_H_
#define AIRFE_POSEOPT_CORE_H_

#include "pnp_core.h"   // pnp_gauss, pnp_cayley, pnp_uidx, AIRFE_HD

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define PO_MAX_POINTS 1024
#define PO_LANES 64             // partial sums: partial l takes the constraints l, l + 64, ... in order; the partials are added in lane order
#define PO_ROUNDS 3             // g2o_optimization.cc:726
#define PO_ITERS 10             // optimizer.optimize(its[iter]), its = 10, 10, 10
#define PO_TRIALS 10            // g2o's maxTrialsAfterFailure
#define PO_MIN_EDGES 10         // `if (optimizer.edges().size() < 10) break;` after the first round
#define PO_TAU 1e-5             // g2o's computeLambdaInit: tau * max |H_jj|
#define PO_TRACE 4              // per round: robust chi at the start pose, robust chi at the end, lambda at the end, iterations begun

// constraints in structure-of-arrays form: component k (X, Y, Z, x, y, u_right) of constraint i at cons[k * PO_MAX_POINTS + i]
#define PO_C(cons, k, i) ((cons)[(k) * PO_MAX_POINTS + (i)])

// state S [PO_SIZE] (doubles)
#define PO_RCB 0      // [9] Rcb row-major
#define PO_TCB 9      // [3]
#define PO_TBC 12     // [3] -(Rcb^T tcb)
#define PO_CAM 15     // [5] fx, fy, cx, cy, bf
#define PO_THR 20     // [2] chi-square thresholds mono, stereo
#define PO_DEL 22     // [2] Huber deltas = sqrt(threshold)
#define PO_WB0 24     // [12] Rwb, twb of the start pose
#define PO_WB 36      // [12] Rwb, twb of the current (accepted) pose
#define PO_WBT 48     // [12] Rwb, twb of the trial
#define PO_CUR 60     // [12] Rcw, tcw of the current pose
#define PO_TRY 72     // [12] Rcw, tcw of the trial
#define PO_ACC 84     // [28] sums at the current pose: H (21 upper entries, row-major), sum w J^T e (6; b is its negative), robust chi
#define PO_LAM 112
#define PO_NI 113
#define PO_RHO 114
#define PO_Q 115      // trials of this iteration so far
#define PO_OK 116     // the last solve succeeded
#define PO_NEXT 117   // this iteration's trials are over
#define PO_STOP 118   // this round's optimisation is over
#define PO_DX 119     // [6] the step
#define PO_AUG 125    // [6][7] damped system, then Cay(dr / 2) [9]
#define PO_SIZE 168

// Rcw = Rcb Rwb^T, tcw = tcb - Rcw twb (VIPose::Update's last lines) from wb [12] into cw [12]
AIRFE_HD void po_camera(const double* S, const double* wb, double* cw) {
  const double* Rcb = S + PO_RCB;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) cw[3 * r + c] = (Rcb[3 * r] * wb[3 * c] + Rcb[3 * r + 1] * wb[3 * c + 1]) + Rcb[3 * r + 2] * wb[3 * c + 2];
  for (int r = 0; r < 3; ++r) cw[9 + r] = S[PO_TCB + r] - ((cw[3 * r] * wb[9] + cw[3 * r + 1] * wb[10]) + cw[3 * r + 2] * wb[11]);
}

// Twc0 [16] row-major, Tcb [12] (Rcb row-major, tcb) or NULL = identity, cam [5], thr [2]
AIRFE_HD void po_init(double* S, const double* Twc0, const double* Tcb, const double* cam, const double* thr) {
  for (int k = 0; k < 9; ++k) S[PO_RCB + k] = Tcb ? Tcb[k] : ((k % 4) == 0 ? 1.0 : 0.0);
  for (int k = 0; k < 3; ++k) S[PO_TCB + k] = Tcb ? Tcb[9 + k] : 0.0;
  const double* Rcb = S + PO_RCB;
  const double* tcb = S + PO_TCB;
  for (int r = 0; r < 3; ++r) S[PO_TBC + r] = -((Rcb[r] * tcb[0] + Rcb[3 + r] * tcb[1]) + Rcb[6 + r] * tcb[2]);
  for (int k = 0; k < 5; ++k) S[PO_CAM + k] = cam[k];
  for (int k = 0; k < 2; ++k) { S[PO_THR + k] = thr[k]; S[PO_DEL + k] = sqrt(thr[k]); }
  // Twb = Twc Tcb
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) S[PO_WB0 + 3 * r + c] = (Twc0[4 * r] * Rcb[c] + Twc0[4 * r + 1] * Rcb[3 + c]) + Twc0[4 * r + 2] * Rcb[6 + c];
    S[PO_WB0 + 9 + r] = ((Twc0[4 * r] * tcb[0] + Twc0[4 * r + 1] * tcb[1]) + Twc0[4 * r + 2] * tcb[2]) + Twc0[4 * r + 3];
  }
}
// every round starts from the start pose (g2o_optimization.cc:727)
AIRFE_HD void po_round_start(double* S) {
  for (int k = 0; k < 12; ++k) S[PO_WB + k] = S[PO_WB0 + k];
  po_camera(S, S + PO_WB, S + PO_CUR);
  S[PO_STOP] = 0.0;
}

// the error of constraint i at the pose Rt (Rcw, tcw): e [3] (e[2] = 0 for a mono edge), Xc [3], 1/z; returns chi2 = e.e; *stereo = u_right > 0
AIRFE_HD double po_error(const double* Rt, const double* S, const double* cons, int i, double* e, double* Xc, double* izp, bool* stereo) {
  const double X = PO_C(cons, 0, i), Y = PO_C(cons, 1, i), Z = PO_C(cons, 2, i);
  const double x = PO_C(cons, 3, i), y = PO_C(cons, 4, i), ur = PO_C(cons, 5, i);
  const double xc = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[9];
  const double yc = Rt[3] * X + Rt[4] * Y + Rt[5] * Z + Rt[10];
  const double zc = Rt[6] * X + Rt[7] * Y + Rt[8] * Z + Rt[11];
  const double iz = 1.0 / zc;
  const double u = xc * iz * S[PO_CAM] + S[PO_CAM + 2], v = yc * iz * S[PO_CAM + 1] + S[PO_CAM + 3];
  const bool st = ur > 0.0;
  const double e0 = x - u, e1 = y - v;
  double e2 = 0.0;
  if (st) e2 = ur - (u - S[PO_CAM + 4] * iz);
  e[0] = e0; e[1] = e1; e[2] = e2;
  Xc[0] = xc; Xc[1] = yc; Xc[2] = zc;
  *izp = iz;
  *stereo = st;
  return (e0 * e0 + e1 * e1) + e2 * e2;
}
AIRFE_HD double po_chi2(const double* Rt, const double* S, const double* cons, int i, bool* stereo) {
  double e[3], Xc[3], iz;
  return po_error(Rt, S, cons, i, e, Xc, &iz, stereo);
}
// g2o's RobustKernelHuber: rho and its derivative w
AIRFE_HD double po_huber(double chi2, double delta, double* w) {
  if (chi2 <= delta * delta) { *w = 1.0; return chi2; }
  const double s = sqrt(chi2);
  *w = delta / s;
  return 2.0 * s * delta - delta * delta;
}
// the robust chi of constraint i alone (a trial's cost)
AIRFE_HD double po_edge_chi(const double* Rt, const double* S, const double* cons, int i) {
  bool st;
  double w;
  const double chi2 = po_chi2(Rt, S, cons, i, &st);
  return po_huber(chi2, S[PO_DEL + (st ? 1 : 0)], &w);
}
// acc [28] += w J^T J (21), w J^T e (6), rho of constraint i at the pose Rt.  J = P Rcb [ -[Xb]x | I ] (3 x 6; the third row is zero for a mono edge)
AIRFE_HD void po_edge_full(const double* Rt, const double* S, const double* cons, int i, double* acc) {
  double e[3], Xc[3], iz, w;
  bool st;
  const double chi2 = po_error(Rt, S, cons, i, e, Xc, &iz, &st);
  const double rho = po_huber(chi2, S[PO_DEL + (st ? 1 : 0)], &w);
  const double* Rcb = S + PO_RCB;
  const double fx = S[PO_CAM], fy = S[PO_CAM + 1], bf = S[PO_CAM + 4];
  const double a = Xc[0] * iz, b = Xc[1] * iz;
  const double p00 = fx * iz, p02 = -(fx * a * iz), p11 = fy * iz, p12 = -(fy * b * iz);
  const double p22 = p02 + bf * (iz * iz);
  double Xb[3];
  for (int r = 0; r < 3; ++r) Xb[r] = ((Rcb[r] * Xc[0] + Rcb[3 + r] * Xc[1]) + Rcb[6 + r] * Xc[2]) + S[PO_TBC + r];
  double J[18];
  for (int c = 0; c < 3; ++c) {
    J[3 + c] = p00 * Rcb[c] + p02 * Rcb[6 + c];
    J[9 + c] = p11 * Rcb[3 + c] + p12 * Rcb[6 + c];
    double a2 = 0.0;
    if (st) a2 = p00 * Rcb[c] + p22 * Rcb[6 + c];
    J[15 + c] = a2;
  }
  for (int r = 0; r < 3; ++r) {
    const double a0 = J[6 * r + 3], a1 = J[6 * r + 4], a2 = J[6 * r + 5];
    J[6 * r] = a2 * Xb[1] - a1 * Xb[2];
    J[6 * r + 1] = a0 * Xb[2] - a2 * Xb[0];
    J[6 * r + 2] = a1 * Xb[0] - a0 * Xb[1];
  }
  if (!st)
    for (int c = 0; c < 3; ++c) J[12 + c] = 0.0;       // (a NaN point must not reach a mono edge's sums through 0 * NaN)
  int m = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < 6; ++r)
#if defined(__clang__)
#pragma unroll
#endif
    for (int c = r; c < 6; ++c) {
      acc[m] = acc[m] + w * ((J[r] * J[c] + J[6 + r] * J[6 + c]) + J[12 + r] * J[12 + c]);
      ++m;
    }
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < 6; ++r) acc[21 + r] = acc[21 + r] + w * ((J[r] * e[0] + J[6 + r] * e[1]) + J[12 + r] * e[2]);
  acc[27] = acc[27] + rho;
}
// the 64 partials p[l * stride] added in lane order
AIRFE_HD double po_sum_lanes(const double* p, int stride) {
  double s = 0.0;
  for (int l = 0; l < PO_LANES; ++l) s = s + p[l * stride];
  return s;
}

// ---- g2o's OptimizationAlgorithmLevenberg::solve, one iteration split at its cost evaluations ------------------------------------------------------
// tot [28]: the sums at the current pose
AIRFE_HD void po_iter_begin(double* S, const double* tot, int it) {
  for (int k = 0; k < 28; ++k) S[PO_ACC + k] = tot[k];
  if (it == 0) {
    double mx = 0.0;
    for (int j = 0; j < 6; ++j) {
      const double d = fabs(tot[pnp_uidx(j, j)]);
      mx = d > mx ? d : mx;
    }
    S[PO_LAM] = PO_TAU * mx;
    S[PO_NI] = 2.0;
  }
  S[PO_Q] = 0.0;
  S[PO_NEXT] = 0.0;
}
// (H + lambda I) dx = b; the trial pose Rwb Cay(dr / 2), twb + Rwb dt.  A failed solve leaves dx = 0 and PO_OK = 0.
AIRFE_HD void po_propose(double* S) {
  double* N = S + PO_AUG;
  const double lam = S[PO_LAM];
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) {
      const double a = S[PO_ACC + (r <= c ? pnp_uidx(r, c) : pnp_uidx(c, r))];
      N[7 * r + c] = r == c ? a + lam : a;
    }
    N[7 * r + 6] = -S[PO_ACC + 21 + r];
  }
  double* d = S + PO_DX;
  const bool ok = pnp_gauss(N, 6, d);
  S[PO_OK] = ok ? 1.0 : 0.0;
  if (!ok)
    for (int k = 0; k < 6; ++k) d[k] = 0.0;
  double* C = N;
  pnp_cayley(d[0] / 2.0, d[1] / 2.0, d[2] / 2.0, C);
  const double* R = S + PO_WB;
  double* T = S + PO_WBT;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[3 * r + c] = (R[3 * r] * C[c] + R[3 * r + 1] * C[3 + c]) + R[3 * r + 2] * C[6 + c];
    T[9 + r] = R[9 + r] + ((R[3 * r] * d[3] + R[3 * r + 1] * d[4]) + R[3 * r + 2] * d[5]);
  }
  po_camera(S, T, S + PO_TRY);
}
// the trial's verdict.  chi_new: the robust chi at the trial pose
AIRFE_HD void po_judge(double* S, double chi_new) {
  if (S[PO_OK] == 0.0) chi_new = INFINITY;
  const double lam = S[PO_LAM];
  const double* d = S + PO_DX;
  double scale = 0.0;
  for (int j = 0; j < 6; ++j) scale = scale + d[j] * (lam * d[j] + (-S[PO_ACC + 21 + j]));
  scale = scale + 1e-3;
  const double rho = (S[PO_ACC + 27] - chi_new) / scale;
  S[PO_RHO] = rho;
  bool brk = false;
  if (rho > 0.0 && isfinite(chi_new)) {
    const double x = 2.0 * rho - 1.0;
    double alpha = 1.0 - (x * x) * x;
    alpha = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;
    const double f = (1.0 / 3.0) < alpha ? alpha : (1.0 / 3.0);
    S[PO_LAM] = lam * f;
    S[PO_NI] = 2.0;
    S[PO_ACC + 27] = chi_new;
    for (int k = 0; k < 12; ++k) { S[PO_WB + k] = S[PO_WBT + k]; S[PO_CUR + k] = S[PO_TRY + k]; }
  } else {
    S[PO_LAM] = lam * S[PO_NI];
    S[PO_NI] = S[PO_NI] * 2.0;
    brk = !isfinite(S[PO_LAM]);
  }
  if (!brk) S[PO_Q] = S[PO_Q] + 1.0;
  const bool again = !brk && rho < 0.0 && S[PO_Q] < (double)PO_TRIALS;
  if (!again) {
    S[PO_NEXT] = 1.0;
    if (S[PO_Q] == (double)PO_TRIALS || rho == 0.0 || !isfinite(S[PO_LAM])) S[PO_STOP] = 1.0;
  }
}
// outlier (level 1) iff the chi2, rounded to float, exceeds the threshold
AIRFE_HD bool po_outlier(const double* Rt, const double* S, const double* cons, int i) {
  bool st;
  const double chi2 = po_chi2(Rt, S, cons, i, &st);
  return (double)(float)chi2 > S[PO_THR + (st ? 1 : 0)];
}
AIRFE_HD bool po_finite12(const double* p) {
  bool f = true;
  for (int k = 0; k < 12; ++k) f = f && isfinite(p[k]);
  return f;
}
// Twc = Twb Tbc (16, row-major) of the current pose
AIRFE_HD void po_twc(const double* S, double* T) {
  const double* W = S + PO_WB;
  const double* Rcb = S + PO_RCB;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[4 * r + c] = (W[3 * r] * Rcb[3 * c] + W[3 * r + 1] * Rcb[3 * c + 1]) + W[3 * r + 2] * Rcb[3 * c + 2];
    T[4 * r + 3] = ((W[3 * r] * S[PO_TBC] + W[3 * r + 1] * S[PO_TBC + 1]) + W[3 * r + 2] * S[PO_TBC + 2]) + W[9 + r];
    T[12 + r] = 0.0;
  }
  T[15] = 1.0;
}

// ---- the tracking composite's seed (map_builder.cc:310-314): the PnP pose, or the last tracked pose when it jumps > 1 m or has too few inliers ------
AIRFE_HD bool po_use_last(const double* Tpnp, int pnp_count, double lx, double ly, double lz, int lost_num_match) {
  const double dx = Tpnp[3] - lx, dy = Tpnp[7] - ly, dz = Tpnp[11] - lz;
  return sqrt((dx * dx + dy * dy) + dz * dz) > 1.0 || pnp_count < lost_num_match;
}

// ---- the host core: the whole contract for one problem, serially (the kernel computes the same bits) ---------------------------------------------
// X [n][3], obs [n][3] (x, y, u_right); cam [5]; Tcb [12] or NULL; thr [2]; Twc0 [16].  Outputs: Twc [16], Rt [12] (Rcw row-major, tcw; may be NULL),
// inlier [n], *num; trace [PO_ROUNDS][PO_TRACE] (may be NULL; zeros for a round that did not run).  Returns the rounds run.
inline int poseopt_solve_host(const double* X, const double* obs, int n, const double* cam, const double* Tcb, const double* thr, const double* Twc0,
                              double* Twc, double* Rt, uint8_t* inlier, int* num, double* trace) {
  double cons[6 * PO_MAX_POINTS], S[PO_SIZE], part[PO_LANES * 28], tot[28];
  uint8_t lvl[PO_MAX_POINTS];
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) { PO_C(cons, k, i) = X[3 * i + k]; PO_C(cons, 3 + k, i) = obs[3 * i + k]; }
    lvl[i] = 0;
  }
  if (trace)
    for (int k = 0; k < PO_ROUNDS * PO_TRACE; ++k) trace[k] = 0.0;
  po_init(S, Twc0, Tcb, cam, thr);
  po_round_start(S);
  int rounds = 0, outliers = 0;
  for (int round = 0; round < PO_ROUNDS && n > 0; ++round) {
    po_round_start(S);
    ++rounds;
    for (int it = 0; it < PO_ITERS; ++it) {
      for (int k = 0; k < PO_LANES * 28; ++k) part[k] = 0.0;
      for (int l = 0; l < PO_LANES; ++l)
        for (int i = l; i < n; i += PO_LANES)
          if (!lvl[i]) po_edge_full(S + PO_CUR, S, cons, i, part + 28 * l);
      for (int k = 0; k < 28; ++k) tot[k] = po_sum_lanes(part + k, 28);
      po_iter_begin(S, tot, it);
      if (trace) {
        if (it == 0) trace[PO_TRACE * round] = tot[27];
        trace[PO_TRACE * round + 3] = (double)(it + 1);
      }
      while (S[PO_NEXT] == 0.0) {
        po_propose(S);
        for (int l = 0; l < PO_LANES; ++l) {
          double c = 0.0;
          for (int i = l; i < n; i += PO_LANES)
            if (!lvl[i]) c = c + po_edge_chi(S + PO_TRY, S, cons, i);
          part[l] = c;
        }
        po_judge(S, po_sum_lanes(part, 1));
      }
      if (S[PO_STOP] != 0.0) break;
    }
    if (trace) { trace[PO_TRACE * round + 1] = S[PO_ACC + 27]; trace[PO_TRACE * round + 2] = S[PO_LAM]; }
    outliers = 0;
    for (int i = 0; i < n; ++i) {
      lvl[i] = po_outlier(S + PO_CUR, S, cons, i) ? 1 : 0;
      outliers += lvl[i];
    }
    if (n < PO_MIN_EDGES) break;
  }
  const bool good = n > 0 && po_finite12(S + PO_WB);
  if (good) {
    po_twc(S, Twc);
  } else {
    for (int k = 0; k < 16; ++k) Twc[k] = Twc0[k];
    po_round_start(S);
  }
  if (Rt)
    for (int k = 0; k < 12; ++k) Rt[k] = canon_nan(S[PO_CUR + k]);
  for (int i = 0; i < n; ++i) inlier[i] = (good && !lvl[i]) ? 1 : 0;
  *num = good ? n - outliers : 0;
  return rounds;
}

#endif  // AIRFE_POSEOPT_CORE_H_
