// airfe — relocalisation's junction term: Frame::FindJunctionConnections (src/frame.cc:581-629) and the counts of MapUser::Relocalization
// (src/map_user.cc:285-331) on plain arrays.  Contract: include/airfe.h ("Junction term").  One statement for the host and the device: the kernels
// (kernels_junction.hip) call the AIRFE_HD routines below from their lanes, the *_host routines at the end call them in loops; tests/junction_ref.py restates
// the reference literally (dense H x W map, std::set, inverted file, match_matrix, four nested loops).
//   pixel(i)      ((int)((double)jx + 0.5), (int)((double)jy + 0.5)) of junction row i = (score, jx, jy, ...); outside [0, W) x [0, H): owns no cell
//   owner(r, c)   the HIGHEST index i with pixel(i) = (c, r)  (the reference writes its map in index order)
//   match(ex, ey) the owner of the cell with the smallest key (|yi - r| + |xi - c|, r, c) over |yi - r| <= 2, |xi - c| <= 2, or -1
//   edges         per line with both ends matched to a, b: (a, b) and (b, a); the distinct ones, ascending by (a, b)
//   word table    the distinct valid words of a frame, ascending, each with cnt (junctions holding it) and conn (those of them with >= 1 edge)
//   key table     the distinct word[a] << 32 | word[b] over the edges with both words valid, ascending, each with its multiplicity
//   match_num     sum over words w of conn_q(w) * cnt_f(w);   line_match_num = sum over keys k of n_q(k) * n_f(k)
//   extra         score * (1.0 + (match_num > 0 ? (double)line_match_num / match_num : 0))
// Integers except the last line; an invalid word (UINT_MAX) enters no table, so invalid words never match each other.
#ifndef AIRFE_JUNCTION_CORE_H_
#define AIRFE_JUNCTION_CORE_H_

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "core_common.h"

#define JN_MAX_JUNCTIONS 1024        // junctions per frame (= BOW_MAX_FEATURES: the BoW kernels' limit)
#define JN_MAX_EDGES 4096            // distinct directed edges per frame (ecap <= this): the products of the term fit int32
#define JN_WS 2                      // frame.cc:593
#define JN_NO_WORD 0xFFFFFFFFu       // database.cc:75
#define JN_NO_PIXEL (-2147483647 - 1)
#define JN_OK 0
#define JN_UNSET 1                   // a stored frame without junction state
#define JN_OVERFLOW 2                // more than ecap distinct edges (or more than 1024 junctions): no edges, a term of 0


// int(v + 0.5) as the reference computes it (a double sum, truncated towards zero); false where that conversion is undefined
AIRFE_HD bool jn_cell(double v, int* out) {
  const double t = v + 0.5;
  if (!(t > -2147483648.0 && t < 2147483648.0)) return false;       // NaN, infinities and everything outside int
  *out = (int)t;
  return true;
}

// frame.cc:588-590 for one junction row; *x = JN_NO_PIXEL where the junction owns no cell
AIRFE_HD void jn_pixel(const float* row, int W, int H, int* x, int* y) {
  int px = 0, py = 0;
  if (jn_cell((double)row[1], &px) && jn_cell((double)row[2], &py) && px >= 0 && px < W && py >= 0 && py < H) { *x = px; *y = py; return; }
  *x = JN_NO_PIXEL;
  *y = JN_NO_PIXEL;
}

// frame.cc:594-617 over the junctions' pixels instead of the dense map: the row-major scan with a strict < keeps the first cell of the smallest distance,
// i.e. the smallest (d, r, c); a cell shared by several junctions belongs to the highest index
AIRFE_HD int jn_match(const int* px, const int* py, int nj, double ex, double ey) {
  int xi = 0, yi = 0;
  if (!jn_cell(ex, &xi) || !jn_cell(ey, &yi)) return -1;
  int best = -1, bd = 2 * JN_WS + 1, br = 0, bc = 0;
  for (int i = 0; i < nj; ++i) {
    const int c = px[i], r = py[i];
    if (c == JN_NO_PIXEL) continue;
    const long long dy = (long long)yi - r, dx = (long long)xi - c;
    if (dy < -JN_WS || dy > JN_WS || dx < -JN_WS || dx > JN_WS) continue;
    const int d = (int)(dy < 0 ? -dy : dy) + (int)(dx < 0 ? -dx : dx);
    if (best < 0 || d < bd || (d == bd && (r < br || (r == br && c <= bc)))) { best = i; bd = d; br = r; bc = c; }
  }
  return best;
}

AIRFE_HD unsigned jn_edge_key(int a, int b) { return ((unsigned)a << 16) | (unsigned)b; }
AIRFE_HD unsigned long long jn_word_key(unsigned wa, unsigned wb) { return ((unsigned long long)wa << 32) | wb; }
// is (a, b) an edge between two junctions of the frame?  (an edge list handed in by a caller is read with this guard)
AIRFE_HD bool jn_edge_ok(int a, int b, int nj) { return a >= 0 && a < nj && b >= 0 && b < nj; }

// position of `w` in an ascending table of n distinct entries, or -1
template <class T>
AIRFE_HD int jn_find(const T* tab, int n, T w) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] < w) lo = mid + 1; else hi = mid;
  }
  return lo < n && tab[lo] == w ? lo : -1;
}

// map_user.cc:329-331: one division, one add, one multiply (the kernel file is compiled with -ffp-contract=off)
AIRFE_HD double jn_extra(double score, int match_num, int line_match_num) {
  const double rate = match_num > 0 ? (double)line_match_num / match_num : 0;
  return score * (1.0 + rate);
}

// ---- the host statements --------------------------------------------------------------------------------------------------------------------------
// lines [nl][4] f64, junc [nj][259] f32 -> edge i32 [ecap][2] ascending, *nedge, line_pair i32 [nl][2] (or nullptr).  Returns the frame's status.
inline int jn_connections_host(const double* lines, int nl, const float* junc, int nj, int W, int H, int32_t* edge, int ecap, int* nedge, int32_t* line_pair) {
  *nedge = 0;
  if (nl < 0) nl = 0;
  if (line_pair) std::fill(line_pair, line_pair + (size_t)nl * 2, -1);
  if (nj > JN_MAX_JUNCTIONS) return JN_OVERFLOW;
  if (nj < 0) nj = 0;
  std::vector<int> px((size_t)nj + 1), py((size_t)nj + 1);
  for (int i = 0; i < nj; ++i) jn_pixel(junc + (size_t)i * 259, W, H, &px[i], &py[i]);
  std::vector<unsigned> keys;
  for (int l = 0; l < nl; ++l) {
    const double* p = lines + (size_t)l * 4;
    const int a = jn_match(px.data(), py.data(), nj, p[0], p[1]);
    if (a < 0) continue;
    const int b = jn_match(px.data(), py.data(), nj, p[2], p[3]);
    if (b < 0) continue;
    if (line_pair) { line_pair[2 * l] = a; line_pair[2 * l + 1] = b; }
    keys.push_back(jn_edge_key(a, b));
    keys.push_back(jn_edge_key(b, a));
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  if ((long long)keys.size() > ecap) return JN_OVERFLOW;
  for (size_t e = 0; e < keys.size(); ++e) { edge[2 * e] = (int32_t)(keys[e] >> 16); edge[2 * e + 1] = (int32_t)(keys[e] & 0xFFFFu); }
  *nedge = (int)keys.size();
  return JN_OK;
}

// word [nj] u32, edge [ne][2] -> the word table uword / wcnt / wconn [<= nj] + *nuw, the key table ukey / kcnt [<= ne] + *nuk
inline void jn_keys_host(const uint32_t* word, int nj, const int32_t* edge, int ne, uint32_t* uword, int32_t* wcnt, int32_t* wconn, int* nuw,
                         unsigned long long* ukey, int32_t* kcnt, int* nuk) {
  std::vector<char> conn((size_t)nj + 1, 0);
  std::vector<unsigned long long> keys;
  for (int e = 0; e < ne; ++e) {
    const int a = edge[2 * e], b = edge[2 * e + 1];
    if (!jn_edge_ok(a, b, nj)) continue;
    conn[a] = 1;
    if (word[a] != JN_NO_WORD && word[b] != JN_NO_WORD) keys.push_back(jn_word_key(word[a], word[b]));
  }
  std::vector<unsigned long long> ws;                              // (word, junction) like the vector kernel's sort keys
  for (int i = 0; i < nj; ++i)
    if (word[i] != JN_NO_WORD) ws.push_back(jn_word_key(word[i], (unsigned)i));
  std::sort(ws.begin(), ws.end());
  int u = 0;
  for (size_t p = 0; p < ws.size(); ++p) {
    const unsigned w = (unsigned)(ws[p] >> 32);
    if (p == 0 || (unsigned)(ws[p - 1] >> 32) != w) { uword[u] = w; wcnt[u] = 0; wconn[u] = 0; ++u; }
    ++wcnt[u - 1];
    wconn[u - 1] += conn[(unsigned)ws[p]];
  }
  *nuw = u;
  std::sort(keys.begin(), keys.end());
  int k = 0;
  for (size_t p = 0; p < keys.size(); ++p) {
    if (p == 0 || keys[p - 1] != keys[p]) { ukey[k] = keys[p]; kcnt[k] = 0; ++k; }
    ++kcnt[k - 1];
  }
  *nuk = k;
}

// the counts of one (query, frame) pair from the two sides' tables
inline void jn_term_host(const uint32_t* q_uword, const int32_t* q_wconn, int q_nuw, const unsigned long long* q_ukey, const int32_t* q_kcnt, int q_nuk,
                         const uint32_t* f_uword, const int32_t* f_wcnt, int f_nuw, const unsigned long long* f_ukey, const int32_t* f_kcnt, int f_nuk,
                         int* match_num, int* line_match_num) {
  int mn = 0, lmn = 0;
  for (int e = 0; e < f_nuw; ++e) {
    const int s = jn_find(q_uword, q_nuw, f_uword[e]);
    if (s >= 0) mn += q_wconn[s] * f_wcnt[e];
  }
  for (int e = 0; e < f_nuk; ++e) {
    const int s = jn_find(q_ukey, q_nuk, f_ukey[e]);
    if (s >= 0) lmn += q_kcnt[s] * f_kcnt[e];
  }
  *match_num = mn;
  *line_match_num = lmn;
}

#endif  // AIRFE_JUNCTION_CORE_H_
