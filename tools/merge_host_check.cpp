// The host statement of the map-point merge (airslam_amd/csrc/merge_core.h) on a planted table whose every buffer is a heap block of exactly the size the
// contract gives it, so that a sanitizer sees any read or write past one.  Stand-alone: no GPU, no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iairslam_amd/csrc tools/merge_host_check.cpp -o merge_host_check
//   ./merge_host_check        (prints the info words and "ok"; a non-zero exit is a finding)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "merge_core.h"

template <class T>
static std::unique_ptr<T[]> block(size_t count) { return std::unique_ptr<T[]>(new T[count]); }

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

int main() {
  const int frames = 6, size = 5, cap = 8, feat_dim = 3, P = 40, Q = 5, mcap = 4;
  auto ids = block<int32_t>((size_t)frames * cap);
  auto xyz = block<double>((size_t)frames * cap * 3);
  auto feat = block<float>((size_t)frames * cap * feat_dim);
  auto n = block<int>(frames);
  for (int r = 0; r < frames * cap; ++r) {
    ids[r] = -1;
    xyz[3 * r] = xyz[3 * r + 1] = xyz[3 * r + 2] = quiet_nan();
    feat[3 * r] = 0.f; feat[3 * r + 1] = 20.f + 7.f * (r % 11); feat[3 * r + 2] = 15.f + 5.f * (r % 13);
  }
  const int counts[frames] = {8, 8, 5, 8, 0, 8};
  for (int f = 0; f < frames; ++f) n[f] = counts[f];
  auto put = [&](int f, int i, int m, bool tri) {
    ids[f * cap + i] = m;
    if (tri) { xyz[3 * (f * cap + i)] = 1.0 + m; xyz[3 * (f * cap + i) + 1] = 2.0; xyz[3 * (f * cap + i) + 2] = 3.0 + f; }
  };
  put(0, 0, 10, true); put(0, 7, 11, false); put(0, 3, P - 1, true); put(1, 0, 12, true); put(1, 7, 13, true); put(2, 4, 14, false); put(2, 6, 15, true);
  put(3, 7, 16, true); put(3, 1, 38, false); put(5, 0, 17, true); put(0, 5, 99, true); put(3, 5, -5, false);
  // in play: the last row of a frame, the last frame of the database, the last id, the last list entry of a query, a frame without rows
  auto qframe = block<int32_t>(Q); auto stage = block<int>(Q); auto loop = block<int32_t>(Q); auto nmatch = block<int>(Q);
  auto Rlq = block<double>((size_t)Q * 9); auto tlq = block<double>((size_t)Q * 3);
  auto mask = block<uint8_t>((size_t)Q * mcap); auto idx = block<int32_t>((size_t)Q * mcap * 2);
  for (int q = 0; q < Q; ++q) {
    for (int k = 0; k < 9; ++k) Rlq[9 * q + k] = k % 4 == 0 ? 1.0 : 0.0;
    tlq[3 * q] = -0.3; tlq[3 * q + 1] = 0.05 * q; tlq[3 * q + 2] = 0.1;
    for (int e = 0; e < mcap; ++e) { mask[q * mcap + e] = 1; idx[2 * (q * mcap + e)] = idx[2 * (q * mcap + e) + 1] = -1; }
  }
  auto entry = [&](int q, int e, int qi, int ci, int m) { idx[2 * (q * mcap + e)] = qi; idx[2 * (q * mcap + e) + 1] = ci; mask[q * mcap + e] = (uint8_t)m; };
  qframe[0] = 3; loop[0] = 0; stage[0] = 0; nmatch[0] = 4;            // (3, 7): 16 with 10; (3, 1): 38 with P - 1; (3, 5) adopts 10; an outlier
  entry(0, 0, 7, 0, 1); entry(0, 1, 1, 3, 1); entry(0, 2, 5, 0, 9); entry(0, 3, 7, 0, 0);
  qframe[1] = 3; loop[1] = 1; stage[1] = 0; nmatch[1] = 9;            // nmatch past mcap; (3, 5) adopts 13 too; rows past the counts
  entry(1, 0, 5, 7, 1); entry(1, 1, 8, 0, 1); entry(1, 2, 0, 8, 1); entry(1, 3, 7, 0, 1);
  qframe[2] = 1; loop[2] = 2; stage[2] = 0; nmatch[2] = 3;            // the gate on 14 (no position); row 6 of frame 2 is past its count of 5
  entry(2, 0, 0, 4, 1); entry(2, 1, 7, 6, 1); entry(2, 2, 0, 4, 0);
  qframe[3] = 5; loop[3] = 0; stage[3] = 0; nmatch[3] = 4;            // frame 5 is beyond size
  entry(3, 0, 0, 0, 1);
  qframe[4] = 4; loop[4] = -1; stage[4] = 3; nmatch[4] = -1;
  MergeTables t;
  t.point_id = ids.get(); t.xyz = xyz.get(); t.feat = feat.get(); t.n = n.get(); t.size = size; t.cap = cap; t.feat_dim = feat_dim; t.max_points = P;
  MergeLoop l;
  l.qframe = qframe.get(); l.Q = Q; l.stage = stage.get(); l.loop = loop.get(); l.Rlq = Rlq.get(); l.tlq = tlq.get(); l.mask = mask.get(); l.idx = idx.get();
  l.mcap = mcap; l.nmatch = nmatch.get();
  l.cam[0] = 458.654; l.cam[1] = 457.296; l.cam[2] = 367.215; l.cam[3] = 248.375;
  auto map = block<int32_t>(P);
  auto info = block<int32_t>(MG_INFO);
  merge_build_host(t, l, frames, map.get(), info.get());
  printf("loop form:");
  for (int k = 0; k < MG_INFO; ++k) printf(" %d", info[k]);
  printf("\n");
  EXPECT(info[MG_I_OUTLIER] == 1 && info[MG_I_ADOPTED] == 1);
  EXPECT(map[16] == 10 && map[13] == 10 && map[12] == 10 && map[38] == P - 1 && map[17] == 17);
  EXPECT(ids[3 * cap + 5] == 10 && ids[3 * cap + 7] == -1 && ids[3 * cap + 1] == P - 1);      // frame 3: row 5 adopts 10, the best, so 16 at row 7 is cleared
  EXPECT(ids[1 * cap + 0] == 10 && ids[1 * cap + 7] == -1);          // frame 1: 12 is the smallest member, its row becomes 10; 13 is cleared
  EXPECT(ids[5 * cap + 0] == 17 && ids[0 * cap + 5] == 99);          // beyond size, and an id out of range: as they were
  for (int m = 0; m < P; ++m) EXPECT(map[m] >= 0 && map[m] < P && map[map[m]] == map[m]);
  // the pair form on what is left, with pairs that must be ignored
  const int NP = 5;
  auto pairs = block<int32_t>((size_t)NP * 2);
  const int32_t pl[NP][2] = {{10, 15}, {P, 10}, {-1, 3}, {15, P - 1}, {17, 17}};
  memcpy(pairs.get(), pl, sizeof(pl));
  merge_pairs_host(t, pairs.get(), NP, map.get(), info.get());
  printf("pair form:");
  for (int k = 0; k < MG_INFO; ++k) printf(" %d", info[k]);
  printf("\n");
  EXPECT(info[MG_I_LIVE] == 3 && info[MG_I_OUTLIER] == 2 && info[MG_I_GROUPS] == 1 && info[MG_I_REMOVED] == 2);
  EXPECT(map[15] == 10 && map[P - 1] == 10 && map[17] == 17);
  merge_pairs_host(t, nullptr, 0, map.get(), info.get());            // no pair: nothing changes
  EXPECT(info[MG_I_GROUPS] == 0 && map[15] == 15);
  printf("ok\n");
  return 0;
}
