// Definitions behind the stand-in headers of shim/stubs/ (test infrastructure; see Eigen/Core for why they exist).
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>

#include "utils.h"

// ---- the four path helpers of the reference's src/utils.cc:177-211 (behaviour restated: regular file / directory tests, '/'-joined path)
bool FileExists(const std::string& file) {
  struct stat st;
  return stat(file.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}
bool PathExists(const std::string& path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
void ConcatenateFolderAndFileName(const std::string& folder, const std::string& file_name, std::string* path) {
  *path = folder;
  if (path->empty() || path->back() != '/') *path += '/';
  *path += file_name;
}
std::string ConcatenateFolderAndFileName(const std::string& folder, const std::string& file_name) {
  std::string p;
  ConcatenateFolderAndFileName(folder, file_name, &p);
  return p;
}

// ---- cv::findFundamentalMat(points0, points1, FM_RANSAC, 20, 0.99, mask): the project's restatement of OpenCV's legacy FM_RANSAC path (the contract in
// include/airfe.h, "F-matrix RANSAC"; per-sample arithmetic shared with the HIP kernels: airslam_amd/csrc/fransac_core.h), run SEQUENTIALLY here as OpenCV
// runs it.  Not OpenCV's numerics: what the tests pin with it is the reference's own glue around the call (the int truncation of cv::Point, the > 8 gate, the
// order-preserving compaction), not OpenCV.
#include <algorithm>
#include <vector>

#include "../../airslam_amd/csrc/fransac_core.h"

// xy [n][4] = (x0, y0, x1, y1); mask [n]; F [9] (may be NULL; zeros when no model); sel (may be NULL) = 3 * sample + root of the selected model, -1 none.
// Returns the number of inliers kept (0: no model).
extern "C" int mini_cv_fundamental_ransac(const double* xy, int n, unsigned char* mask, double* Fout, int* sel) {
  const bool lmeds = n < FR_MIN_RANSAC;
  int niters = lmeds ? FR_LMEDS_ITERS : FR_RANSAC_ITERS, best = -1, bestc = 6;
  float bestmed = INFINITY;
  double bestF[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<float> err(n);
  for (int s = 0; s < niters; ++s) {
    double X[7][4], F[3][9];
    const int m = fr_sample(xy, n, s, X) ? fr_solve7(X, F) : 0;
    for (int r = 0; r < m; ++r) {
      for (int i = 0; i < n; ++i) err[i] = fr_error(F[r], xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3]);
      bool take = false;
      if (!lmeds) {
        int c = 0;
        for (int i = 0; i < n; ++i) c += err[i] <= FR_THRESH2;
        if (c > bestc) { bestc = c; take = true; niters = fr_update_niters(n, c); }
      } else {
        std::vector<float> e(err);
        std::sort(e.begin(), e.end());
        if (e[n / 2] < bestmed) { bestmed = e[n / 2]; take = true; }
      }
      if (take) { best = 3 * s + r; std::copy(F[r], F[r] + 9, bestF); }
    }
  }
  int kept = 0;
  if (best >= 0) {
    const float thr = lmeds ? fr_lmeds_thresh(n, bestmed) : FR_THRESH2;
    for (int i = 0; i < n; ++i) {
      mask[i] = fr_error(bestF, xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3]) <= thr;
      kept += mask[i];
    }
    if (lmeds && kept < 7) best = -1;                       // LMedS reports failure below 7 inliers
  }
  if (best < 0) {
    kept = 0;
    std::fill(mask, mask + n, (unsigned char)0);
    std::fill(bestF, bestF + 9, 0.0);
  }
  if (Fout) std::copy(bestF, bestF + 9, Fout);
  if (sel) *sel = best;
  return kept;
}

namespace cv {
Mat findFundamentalMat(const std::vector<Point>& points1, const std::vector<Point>& points2, int method, double ransacReprojThreshold, double confidence,
                       std::vector<uchar>& mask) {
  if (method != FM_RANSAC || ransacReprojThreshold != 20 || confidence != 0.99 || points1.size() != points2.size() || points1.size() < 9) {
    std::fprintf(stderr, "mini-OpenCV: cv::findFundamentalMat restates only the reference's call (FM_RANSAC, 20, 0.99, more than 8 pairs)\n");
    std::abort();
  }
  const int n = (int)points1.size();
  std::vector<double> xy((size_t)n * 4);
  for (int i = 0; i < n; ++i) {
    xy[4 * i] = points1[i].x; xy[4 * i + 1] = points1[i].y; xy[4 * i + 2] = points2[i].x; xy[4 * i + 3] = points2[i].y;
  }
  mask.assign(n, 0);
  mini_cv_fundamental_ransac(xy.data(), n, mask.data(), nullptr, nullptr);
  return Mat();
}
}  // namespace cv
