// covis_build_host (airslam_amd/csrc/covis_core.h) over the hand cases of tests/covis_ref.py, as a stand-alone program for a sanitizer build:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iairslam_amd/csrc tools/covis_host_check.cpp -o covis_host_check && ./covis_host_check
// Every buffer is sized exactly (no slack), so a read or write past an end is the sanitizer's to find.  Exit status 0 = every table as written out below.
#include <stdio.h>

#include <climits>

#include "covis_core.h"

struct Case {
  const char* name;
  int cap, size, max_frames, max_points, max_edges;
  std::vector<int32_t> ids;
  std::vector<int> n;
  std::vector<int32_t> row_ptr, nbr, weight, info;
};

static int run(const Case& c) {
  std::vector<int32_t> row_ptr((size_t)c.max_frames + 1, -7), nbr((size_t)c.max_edges, -7), weight((size_t)c.max_edges, -7), info(4, -7);
  covis_build_host(c.ids.data(), c.n.data(), c.size, c.max_frames, c.cap, c.max_points, c.max_edges, row_ptr.data(), nbr.data(), weight.data(), info.data());
  const size_t e = (size_t)row_ptr[c.max_frames];
  nbr.resize(e);
  weight.resize(e);
  const bool ok = row_ptr == c.row_ptr && nbr == c.nbr && weight == c.weight && info == c.info;
  printf("%-16s %s (entries %d, valid %d, ignored %d, status %d)\n", c.name, ok ? "ok" : "WRONG", info[1], info[2], info[3], info[0]);
  return ok ? 0 : 1;
}

int main() {
  const int P = 10;
  const std::vector<Case> cases = {
      {"one_frame", 4, 1, 3, P, 1, {4, 7, -1, 2}, {4}, {0, 1, 1, 1}, {0}, {3}, {0, 1, 3, 0}},
      {"empty", 4, 0, 2, P, 1, {1, 2, 3, 4}, {4}, {0, 0, 0}, {}, {}, {0, 0, 0, 0}},
      {"n_zero", 4, 3, 3, P, 4, {5, 1, -1, -1, 5, 5, 5, 5, 5, 2, -1, -1}, {2, 0, 2}, {0, 2, 2, 4}, {0, 2, 0, 2}, {2, 1, 1, 2}, {0, 4, 4, 0}},
      {"all_minus_one", 3, 3, 4, P, 4, {3, -1, -1, -1, -1, -1, 3, 6, -1}, {3, 3, 3}, {0, 2, 2, 4, 4}, {0, 2, 0, 2}, {1, 1, 1, 2}, {0, 4, 3, 0}},
      {"duplicate_row", 4, 2, 2, P, 4, {8, 1, 8, -1, 8, -1, -1, -1}, {4, 4}, {0, 2, 4}, {0, 1, 0, 1}, {3, 2, 1, 1}, {0, 4, 4, 0}},
      {"edge_ids", 3, 3, 3, P, 9, {0, 9, -1, 9, -1, 0, 0, -1, -1}, {3, 3, 3}, {0, 3, 6, 9}, {0, 1, 2, 0, 1, 2, 0, 1, 2}, {2, 2, 1, 2, 2, 1, 1, 1, 1},
       {0, 9, 5, 0}},
      {"out_of_range", 4, 2, 3, P, 4, {10, 3, -2, -1, 3, INT_MAX, INT_MIN, 10}, {4, 4}, {0, 2, 4, 4}, {0, 1, 0, 1}, {1, 1, 1, 1}, {0, 4, 2, 5}},
      // one entry short: status 1, the count needed, every row_ptr 0, nothing written
      {"overflow", 4, 2, 2, P, 3, {8, 1, 8, -1, 8, -1, -1, -1}, {4, 4}, {0, 0, 0}, {}, {}, {1, 4, 4, 0}},
  };
  int bad = 0;
  for (const Case& c : cases) bad += run(c);
  return bad ? 1 : 0;
}
