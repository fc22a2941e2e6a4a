// triangulate_build_host / triangulate_point_host (airslam_amd/csrc/triangulate_core.h) on a small planted table, as a stand-alone program for a sanitizer build:
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iairslam_amd/csrc tools/triangulate_host_check.cpp \
//       -o triangulate_host_check && ./triangulate_host_check
// Every buffer is sized exactly (no slack), so a read or write past an end is the sanitizer's to find.  Exit status 0 = every planted point recovered, every
// status as planted, the two host routines equal.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <climits>

#include "triangulate_core.h"

int main() {
  const int frames = 6, size = 5, cap = 5, P = 9, dim = 3;          // frame 5 lies past `size`; x, y at columns 1, 2 of a 3-wide row
  const double cam[4] = {400.0, 410.0, 320.0, 240.0};
  double cami[4];
  if (!tr_cam(cam, cami)) return 2;
  const double X[4][3] = {{0.5, -0.25, 6.0}, {-1.0, 0.5, 8.0}, {2.0, 1.0, 5.0}, {0.0, 0.0, 7.0}};
  std::vector<double> pose((size_t)frames * 16, 0.0);
  for (int f = 0; f < frames; ++f) {
    const double a = 0.1 * f, T[16] = {cos(a), 0, sin(a), -2.0 + f, 0, 1, 0, 0.1 * f, -sin(a), 0, cos(a), 0, 0, 0, 0, 1};
    memcpy(&pose[(size_t)f * 16], T, sizeof T);
  }
  // ids: point m < 4 at row m of frames m .. 4 (4, 3, 2, 1 observers... point 3 has two), hostile ids around them
  std::vector<int32_t> ids((size_t)frames * cap, -1);
  std::vector<float> feat((size_t)frames * cap * dim, NAN);
  std::vector<int> n = {5, 5, 4, 5, 5};                             // [size] exactly
  for (int f = 0; f < frames; ++f)
    for (int m = 0; m < 4; ++m) {
      if (f < m) continue;
      const double* T = &pose[(size_t)f * 16];
      const double d[3] = {X[m][0] - T[3], X[m][1] - T[7], X[m][2] - T[11]};
      double c[3];
      for (int r = 0; r < 3; ++r) c[r] = T[r] * d[0] + T[4 + r] * d[1] + T[8 + r] * d[2];
      ids[(size_t)f * cap + m] = m;
      feat[((size_t)f * cap + m) * dim + 1] = (float)(cam[0] * c[0] / c[2] + cam[2]);
      feat[((size_t)f * cap + m) * dim + 2] = (float)(cam[1] * c[1] / c[2] + cam[3]);
    }
  ids[0 * cap + 4] = INT_MAX; ids[1 * cap + 4] = INT_MIN; ids[3 * cap + 4] = P; ids[4 * cap + 4] = 0;      // out of range x 3; point 0 a second time in frame 4
  ids[2 * cap + 4] = 8;                                             // row 4 of frame 2 lies past n[2] = 4: never read
  std::vector<double> xyz((size_t)P * 3, 7.0);
  std::vector<int32_t> status(P, -7), nobs(P, -7), info(4, -7);
  triangulate_build_host(feat.data(), dim, n.data(), pose.data(), ids.data(), size, cap, P, cami, 2, xyz.data(), status.data(), nobs.data(), info.data());
  const int want_nobs[9] = {5, 4, 3, 2, 0, 0, 0, 0, 0}, want_status[9] = {0, 0, 0, 0, -1, -1, -1, -1, -1};
  int bad = 0;
  for (int m = 0; m < P; ++m) {
    bool ok = status[m] == want_status[m] && nobs[m] == want_nobs[m];
    if (status[m] == 0) {
      double e = 0, s = 0;
      for (int k = 0; k < 3; ++k) { e += (xyz[3 * m + k] - X[m][k]) * (xyz[3 * m + k] - X[m][k]); s += X[m][k] * X[m][k]; }
      ok = ok && sqrt(e) < 1e-3 * sqrt(s);
      // the same point through the one-point routine
      std::vector<double> Twc;
      std::vector<float> xy;
      for (int f = m; f < size; ++f) {
        Twc.insert(Twc.end(), &pose[(size_t)f * 16], &pose[(size_t)f * 16] + 16);
        xy.push_back(feat[((size_t)f * cap + m) * dim + 1]);
        xy.push_back(feat[((size_t)f * cap + m) * dim + 2]);
      }
      double one[3];
      ok = ok && triangulate_point_host(cami, Twc.data(), xy.data(), size - m, 2, one) == 0 && memcmp(one, &xyz[3 * m], 24) == 0;
    } else {
      ok = ok && xyz[3 * m] != xyz[3 * m] && xyz[3 * m + 1] != xyz[3 * m + 1] && xyz[3 * m + 2] != xyz[3 * m + 2];
    }
    printf("point %d: status %d, %d observers %s\n", m, status[m], nobs[m], ok ? "ok" : "WRONG");
    bad += !ok;
  }
  if (!(info[0] == 4 && info[1] == 4 && info[2] == 0 && info[3] == 0)) { printf("info WRONG\n"); ++bad; }
  return bad ? 1 : 0;
}
