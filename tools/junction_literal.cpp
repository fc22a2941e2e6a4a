// The caller's path without the device junction term, for tools/junction_timing.py: Frame::FindJunctionConnections and the junction part of
// MapUser::Relocalization restated literally on ONE thread — a dense H x W junction map, std::set connections, an inverted file per word, match_matrix, the
// four nested loops, L1 scoring over two std::map vectors.  Built with g++ -O2 -ffp-contract=off; compared with the device's table before anything is timed.
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <set>
#include <vector>

namespace {

struct Frame {
  std::vector<uint32_t> word;                       // word_of_features, UINT_MAX = weight 0
  std::vector<std::set<int>> connected;
  std::map<uint32_t, double> bow;
};
struct Db {
  int W = 0, H = 0;
  std::vector<Frame> frames;
  std::map<uint32_t, std::map<int, std::vector<int>>> inverted;      // word -> frame -> junctions
};

bool cell(double v, int* out) {
  const double t = v + 0.5;
  if (!(t > -2147483648.0 && t < 2147483648.0)) return false;
  *out = (int)t;
  return true;
}

// the window scan over the dense map: rows, then columns, a strictly smaller Manhattan distance replaces, distance 0 ends the scan
int nearest_owner(const std::vector<std::vector<int>>& owner, int W, int H, double ex, double ey) {
  const int reach = 2;
  int xi, yi;
  if (!cell(ex, &xi) || !cell(ey, &yi)) return -1;
  int found = -1, best = 2 * reach + 1;
  for (int r = std::max(yi - reach, 0); r <= std::min(yi + reach, H - 1); ++r)
    for (int c = std::max(xi - reach, 0); c <= std::min(xi + reach, W - 1); ++c) {
      if (owner[r][c] < 0) continue;
      const int d = std::abs(yi - r) + std::abs(xi - c);
      if (d >= best) continue;
      found = owner[r][c];
      best = d;
      if (d == 0) return found;
    }
  return found;
}

void connections(const double* lines, int nl, const float* junc, int nj, int W, int H, std::vector<std::set<int>>& connected) {
  connected.assign(nj, std::set<int>());
  std::vector<std::vector<int>> junction_map(H, std::vector<int>(W, -1));
  for (int i = 0; i < nj; ++i) {
    int x, y;
    if (!cell((double)junc[(size_t)i * 259 + 1], &x) || !cell((double)junc[(size_t)i * 259 + 2], &y) || x < 0 || x >= W || y < 0 || y >= H) continue;
    junction_map[y][x] = i;
  }
  for (int l = 0; l < nl; ++l) {
    const double* p = lines + (size_t)l * 4;
    const int a = nearest_owner(junction_map, W, H, p[0], p[1]);
    if (a < 0) continue;
    const int b = nearest_owner(junction_map, W, H, p[2], p[3]);
    if (b < 0) continue;
    connected[a].insert(b);
    connected[b].insert(a);
  }
}

double l1_score(const std::map<uint32_t, double>& v1, const std::map<uint32_t, double>& v2) {
  std::map<uint32_t, double>::const_iterator a = v1.begin(), b = v2.begin();
  double score = 0;
  while (a != v1.end() && b != v2.end()) {
    if (a->first == b->first) {
      score += fabs(a->second - b->second) - fabs(a->second) - fabs(b->second);
      ++a;
      ++b;
    } else if (a->first < b->first) {
      a = v1.lower_bound(b->first);
    } else {
      b = v2.lower_bound(a->first);
    }
  }
  return -score / 2.0;
}

void fill_frame(Frame& f, const uint32_t* word, int nj, const uint32_t* ids, const double* vals, int nw) {
  f.word.assign(word, word + nj);
  for (int i = 0; i < nw; ++i) f.bow[ids[i]] = vals[i];
}

}  // namespace

extern "C" void* jl_create(int W, int H) {
  Db* d = new Db();
  d->W = W;
  d->H = H;
  return d;
}
extern "C" void jl_destroy(void* h) { delete (Db*)h; }

// one stored frame: its connections, its vector, its entry in the inverted file
extern "C" void jl_add(void* h, const double* lines, int nl, const float* junc, int nj, const uint32_t* word, const uint32_t* ids, const double* vals, int nw) {
  Db* d = (Db*)h;
  const int f = (int)d->frames.size();
  d->frames.emplace_back();
  Frame& fr = d->frames.back();
  fill_frame(fr, word, nj, ids, vals, nw);
  connections(lines, nl, junc, nj, d->W, d->H, fr.connected);
  for (int i = 0; i < nj; ++i)
    if (word[i] != UINT_MAX) d->inverted[word[i]][f].push_back(i);
}

// one query against the stored frames `frames [n]` (or all of them when frames == nullptr): extra[frame] = score * (1 + rate)
extern "C" void jl_query(void* h, const double* lines, int nl, const float* junc, int nj, const uint32_t* word, const uint32_t* ids, const double* vals, int nw,
                         const int* frames, int n, double* extra) {
  Db* d = (Db*)h;
  Frame q;
  fill_frame(q, word, nj, ids, vals, nw);
  connections(lines, nl, junc, nj, d->W, d->H, q.connected);
  const int total = frames ? n : (int)d->frames.size();
  for (int g = 0; g < total; ++g) {
    const int kf = frames ? frames[g] : g;
    const Frame& f = d->frames[kf];
    // same[i][j]: query junction i and stored junction j hold the same valid word; hits[i]: the stored junctions the inverted file lists for i's word
    std::vector<std::vector<bool>> same(nj, std::vector<bool>(f.word.size(), false));
    std::vector<const std::vector<int>*> hits(nj, nullptr);
    for (int i = 0; i < nj; ++i) {
      if (q.word[i] == UINT_MAX) continue;
      std::map<int, std::vector<int>>& listed = d->inverted[q.word[i]];
      std::map<int, std::vector<int>>::const_iterator at = listed.find(kf);
      if (at == listed.end()) continue;
      hits[i] = &at->second;
      for (size_t k = 0; k < at->second.size(); ++k) same[i][at->second[k]] = true;
    }
    int matched = 0, matched_lines = 0;
    for (int i = 0; i < nj; ++i) {
      if (!hits[i] || hits[i]->empty() || q.connected[i].empty()) continue;
      matched += (int)hits[i]->size();
      for (size_t k = 0; k < hits[i]->size(); ++k) {
        const std::set<int>& theirs = f.connected[(*hits[i])[k]];
        for (std::set<int>::const_iterator mine = q.connected[i].begin(); mine != q.connected[i].end(); ++mine)
          for (std::set<int>::const_iterator other = theirs.begin(); other != theirs.end(); ++other)
            if (same[*mine][*other]) ++matched_lines;
      }
    }
    const double rate = matched > 0 ? (double)matched_lines / matched : 0;
    extra[kf] = l1_score(f.bow, q.bow) * (1 + rate);
  }
}
