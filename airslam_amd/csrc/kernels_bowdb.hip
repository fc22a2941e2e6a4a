// airfe — the BoW keyframe database: Database::FrameToBow to its end, Database::AddFrame / Query / Score and the two callers' sharing-word filters
// (src/bow/database.cc:57-124, src/map_user.cc:135-166, src/map_refiner.cc:97-130), and the best-candidate rule behind the matcher
// (map_user.cc:360-376, map_refiner.cc:213-230).  Contract: include/airfe.h ("BoW keyframe database").  Every floating-point sum is sequential, in the
// order the reference's std::map iteration gives it: no atomics on doubles, no tree reductions; the file is compiled with -ffp-contract=off.
//   bow_vector_kernel     (frame)  sort of (word, feature index) keys in LDS, one sequential sum per distinct word, one ordered total, v / tot
//   bowdb_query_kernel    (query, slice of frames)  the query as a word -> slot table (or its sorted ids, searched) + its values in LDS; a wave takes
//                         one frame at a time: 64 consecutive entries per pass, ballot of the common words, popcount = sharing, the score's terms
//                         added by walking the ballot's set bits in lane order = ascending word id
//   bowdb_select_kernel   (query)  max_sharing over all frames, thr, the filters, order-preserving compaction of the candidates
//   bowdb_topk_kernel     (query)  the project's own ranking: K best scores, ties to the lower frame index
//   bowdb_gather_kernel / bowdb_best_kernel  the composite's glue around the context's LightGlue batch and the F-matrix RANSAC
#include "common.h"
#include "core_common.h"
#include "kernels.h"
#include "wg_prims.h"

namespace airfe {

namespace {

__global__ __launch_bounds__(256) void bow_vector_kernel(BowVecArgs a) {
  __shared__ unsigned long long key[BOW_MAX_FEATURES];
  __shared__ double val[BOW_MAX_FEATURES];
  __shared__ unsigned sid[BOW_MAX_FEATURES];
  __shared__ int scan[4];
  __shared__ double s_tot;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = clamp_count(a.n[b], a.cap);
  const unsigned* word = a.word + (size_t)b * a.cap;
  const int* node = a.node + (size_t)b * a.cap;
  int P = 64;
  while (P < n) P <<= 1;                                     // n <= cap <= BOW_MAX_FEATURES
  for (int i = t; i < P; i += 256) {
    unsigned long long k = ~0ull;
    if (i < n) {
      const unsigned w = word[i];
      if (w != 0xFFFFFFFFu) k = ((unsigned long long)w << 32) | (unsigned)i;      // database.cc:70: only words of weight > 0 enter the vector
    }
    key[i] = k;
  }
  block_sort_asc<256>(key, P);                               // ascending (word, feature index); the keys are distinct
  // segment heads: thread t owns positions 4 t .. 4 t + 3
  int heads = 0;
  for (int p = 4 * t; p < 4 * t + 4 && p < P; ++p) {
    const unsigned long long k = key[p];
    if (k != ~0ull && (p == 0 || (unsigned)(key[p - 1] >> 32) != (unsigned)(k >> 32))) ++heads;
  }
  int nw = 0;
  int slot = block_excl_scan<256>(heads, scan, &nw);
  for (int p = 4 * t; p < 4 * t + 4 && p < P; ++p) {
    const unsigned long long k = key[p];
    if (k == ~0ull) break;
    const unsigned w = (unsigned)(k >> 32);
    if (p != 0 && (unsigned)(key[p - 1] >> 32) == w) continue;
    double s = a.weight[node[(unsigned)k]];                  // BowVector::addWeight: the first weight inserts, the later ones add, ascending feature index
    for (int q = p + 1; q < P && (unsigned)(key[q] >> 32) == w; ++q) s += a.weight[node[(unsigned)key[q]]];
    sid[slot] = w;
    val[slot] = s;
    ++slot;
  }
  __syncthreads();
  if (t == 0) {                                              // BowVector::normalize(L1): one sum in ascending word id
    double tot = 0.0;
    for (int i = 0; i < nw; ++i) tot += fabs(val[i]);
    s_tot = tot;
  }
  __syncthreads();
  const double tot = s_tot;
  unsigned* ids = a.ids + (size_t)b * a.cap;
  double* vals = a.vals + (size_t)b * a.cap;
  for (int i = t; i < nw; i += 256) {
    ids[i] = sid[i];
    vals[i] = tot > 0.0 ? val[i] / tot : val[i];
  }
  if (t == 0) a.nw[b] = nw;
}

// slot of `w` in the query (or -1)
template <bool TABLE>
__device__ __forceinline__ int query_slot(unsigned w, const unsigned short* tab, const unsigned* qi, int nq, int n_words) {
  if (TABLE) {
    if (w >= (unsigned)n_words) return -1;
    const unsigned short s = tab[w];
    return s == 0xFFFF ? -1 : (int)s;
  }
  int lo = 0, hi = nq;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (qi[mid] < w) lo = mid + 1; else hi = mid;
  }
  return lo < nq && qi[lo] == w ? lo : -1;
}

template <bool TABLE>
__global__ __launch_bounds__(256) void bowdb_query_kernel(BowQueryArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* qv = reinterpret_cast<double*>(smem);                                   // [BOW_MAX_FEATURES]
  unsigned* qi = reinterpret_cast<unsigned*>(smem + BOW_MAX_FEATURES * 8);         // [BOW_MAX_FEATURES]
  unsigned short* tab = reinterpret_cast<unsigned short*>(smem + BOW_MAX_FEATURES * 12);   // [n_words] (TABLE)
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nq = clamp_count(a.q_nw[q], a.qcap);
  for (int i = t; i < nq; i += 256) {
    qv[i] = a.q_vals[(size_t)q * a.qcap + i];
    qi[i] = a.q_ids[(size_t)q * a.qcap + i];
  }
  if (TABLE) {
    unsigned* t32 = reinterpret_cast<unsigned*>(tab);
    for (int i = t; i < (a.n_words + 1) / 2; i += 256) t32[i] = 0xFFFFFFFFu;
  }
  __syncthreads();
  if (TABLE) {
    for (int i = t; i < nq; i += 256)
      if (qi[i] < (unsigned)a.n_words) tab[qi[i]] = (unsigned short)i;
    __syncthreads();
  }
  const int f0 = blockIdx.y * a.frames_per_wg, f1 = min(a.N, f0 + a.frames_per_wg);
  for (int f = f0 + wave; f < f1; f += 4) {
    const int nf = clamp_count(a.db_nw[f], a.cap);
    const unsigned* ids = a.db_ids + (size_t)f * a.cap;
    const double* vals = a.db_vals + (size_t)f * a.cap;
    int share = 0;
    double s = 0.0;
    unsigned wn = lane < nf ? ids[lane] : 0xFFFFFFFFu;
    double vn = lane < nf ? vals[lane] : 0.0;
    for (int base = 0; base < nf; base += 64) {
      const unsigned w = wn;
      const double v1 = vn;
      const int e = base + 64 + lane;                         // the next pass's entries are in flight while this one is looked up
      wn = e < nf ? ids[e] : 0xFFFFFFFFu;
      vn = e < nf ? vals[e] : 0.0;
      const int slot = w == 0xFFFFFFFFu ? -1 : query_slot<TABLE>(w, tab, qi, nq, a.n_words);
      unsigned long long m = __ballot(slot >= 0);
      share += __popcll(m);
      while (m) {                                             // L1Scoring::score: the common words in ascending word id, v1 = the frame's value, v2 = the query's
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const double x1 = __shfl(v1, l);
        const double x2 = qv[__shfl(slot, l)];
        s += (fabs(x1 - x2) - fabs(x1)) - fabs(x2);
      }
    }
    if (lane == 0) {
      a.sharing[(size_t)q * a.N + f] = share;
      a.score[(size_t)q * a.N + f] = -s / 2.0;
    }
  }
}

__global__ __launch_bounds__(256) void bowdb_select_kernel(BowSelectArgs a) {
  __shared__ int red[4];
  const int q = blockIdx.x, t = threadIdx.x;
  const int* sh = a.sharing + (size_t)q * a.N;
  const double* sc = a.score + (size_t)q * a.N;
  int m = 0;
  for (int f = t; f < a.N; f += 256) m = max(m, sh[f]);
  const int ms = block_max<256>(m, red);                      // over ALL frames, before the filters (map_user.cc:142-145, map_refiner.cc:104-107)
  if (t == 0) a.max_sharing[q] = ms;
  const float prod = __fmul_rn((float)ms, a.ratio);           // static_cast<int>(max_sharing_words * 0.3f): a float product, truncated
  const int thr = max((int)prod, a.min_words);
  const int limit = a.max_index ? a.max_index[q] : a.N;
  const unsigned* ex = a.exclude ? a.exclude + (size_t)q * a.exclude_words : nullptr;
  int base = 0;
  for (int f0 = 0; f0 < a.N; f0 += 256) {
    const int f = f0 + t;
    bool keep = false;
    int s = 0;
    if (f < a.N) {
      s = sh[f];
      keep = s > 0 && s >= thr && f < limit;                  // (a frame without a common word is absent from frame_sharing_words)
      if (keep && ex) keep = (f >> 5) >= a.exclude_words || !((ex[f >> 5] >> (f & 31)) & 1u);
    }
    int total = 0;
    const int pos = base + block_compact<256>(keep, red, &total);
    if (keep && pos < a.ccap) {
      a.cand_frame[(size_t)q * a.ccap + pos] = f;
      a.cand_sharing[(size_t)q * a.ccap + pos] = s;
      a.cand_score[(size_t)q * a.ccap + pos] = sc[f];
    }
    base += total;
  }
  if (t == 0) a.ncand[q] = base;
}

// (score descending, position ascending): is (s, p) better than (bs, bp)?
__device__ __forceinline__ bool better(double s, int p, double bs, int bp) { return bp < 0 || s > bs || (s == bs && p < bp); }

__global__ __launch_bounds__(64) void bowdb_topk_kernel(BowTopkArgs a) {
  __shared__ double ls[64];
  __shared__ int lp[64];
  __shared__ double s_ps;
  __shared__ int s_pp;
  const int q = blockIdx.x, lane = threadIdx.x;
  const int n = clamp_count(a.ncand[q], a.ccap);
  const double* sc = a.cand_score + (size_t)q * a.ccap;
  const int* fr = a.cand_frame + (size_t)q * a.ccap;
  double ps = 0.0;
  int pp = -1;
  for (int r = 0; r < a.K; ++r) {
    double bs = 0.0;
    int bp = -1;
    for (int p = lane; p < n; p += 64) {
      const double s = sc[p];
      const bool after = r == 0 || s < ps || (s == ps && p > pp);      // not yet taken: behind the previous pick in the ranking
      if (after && better(s, p, bs, bp)) { bs = s; bp = p; }
    }
    ls[lane] = bs;
    lp[lane] = bp;
    __syncthreads();
    if (lane == 0) {
      double ws = 0.0;
      int wp = -1;
      for (int l = 0; l < 64; ++l)
        if (lp[l] >= 0 && better(ls[l], lp[l], ws, wp)) { ws = ls[l]; wp = lp[l]; }
      s_ps = ws;
      s_pp = wp;
      a.top[(size_t)q * a.K + r] = wp >= 0 ? fr[wp] : -1;
      if (a.top_score) a.top_score[(size_t)q * a.K + r] = wp >= 0 ? ws : 0.0;
    }
    __syncthreads();
    ps = s_ps;
    pp = s_pp;
    if (pp < 0) {                                              // the list is exhausted: -1 padding
      if (lane == 0)
        for (int r2 = r + 1; r2 < a.K; ++r2) {
          a.top[(size_t)q * a.K + r2] = -1;
          if (a.top_score) a.top_score[(size_t)q * a.K + r2] = 0.0;
        }
      break;
    }
  }
}

// pair p = q * K + k: f0 = the query's rows, f1 = the candidate's kept rows; a hole (candidate < 0 or not in the database) is an empty pair
__global__ __launch_bounds__(256) void bowdb_gather_kernel(BowGatherArgs a) {
  const int p = blockIdx.x, q = p / a.K;
  const int cand = a.cand[p];
  const bool hole = cand < 0 || cand >= a.N;
  const int n0 = hole ? 0 : clamp_count(a.qn[q], a.cap), n1 = hole ? 0 : clamp_count(a.db_n[cand], a.cap);
  if (threadIdx.x == 0) { a.n0[p] = n0; a.n1[p] = n1; }
  if (hole) return;
  const float* s0 = a.qfeat + (size_t)q * a.cap * 259;
  const float* s1 = a.db_feat + (size_t)cand * a.cap * 259;
  float* d0 = a.f0 + (size_t)p * a.cap * 259;
  float* d1 = a.f1 + (size_t)p * a.cap * 259;
  for (int i = threadIdx.x; i < n0 * 259; i += 256) d0[i] = s0[i];
  for (int i = threadIdx.x; i < n1 * 259; i += 256) d1[i] = s1[i];
}

// map_user.cc:370-373: a candidate replaces the best only with a STRICTLY longer list, from an empty one
__global__ __launch_bounds__(256) void bowdb_best_kernel(BowBestArgs a) {
  __shared__ int s_k, s_n;
  const int q = blockIdx.x, t = threadIdx.x;
  if (t == 0) {
    int bk = -1, bn = 0;
    for (int k = 0; k < a.K; ++k) {
      const int cand = a.cand[q * a.K + k];
      const int nm = cand < 0 || cand >= a.N ? 0 : clamp_count(a.nmatch_all[q * a.K + k], a.mcap);
      if (a.out_nmatch_all) a.out_nmatch_all[q * a.K + k] = nm;
      if (nm > bn) { bn = nm; bk = k; }
    }
    s_k = bk;
    s_n = bn;
    a.best[q] = bk >= 0 ? a.cand[q * a.K + bk] : -1;
    a.nmatch[q] = bn;
  }
  __syncthreads();
  const int bk = s_k, bn = s_n;
  if (bk < 0) return;
  const int32_t* si = a.idx_all + (size_t)(q * a.K + bk) * a.mcap * 2;
  const float* ss = a.score_all + (size_t)(q * a.K + bk) * a.mcap;
  for (int i = t; i < bn; i += 256) {
    a.idx[((size_t)q * a.mcap + i) * 2] = si[2 * i];
    a.idx[((size_t)q * a.mcap + i) * 2 + 1] = si[2 * i + 1];
    a.score[(size_t)q * a.mcap + i] = ss[i];
  }
}

}  // namespace

void launch_bow_vector(const BowVecArgs& a, int B, hipStream_t st) {
  if (B < 1) return;
  hipLaunchKernelGGL(bow_vector_kernel, dim3(B), dim3(256), 0, st, a);
}

size_t bowdb_query_lds(int n_words, bool* table) {
  const size_t need = (size_t)BOW_MAX_FEATURES * 12 + ((size_t)n_words + 1) / 2 * 4;
  *table = n_words <= 65535 && need <= 150 * 1024;           // slots are 16-bit (0xFFFF = none); the CU has 160 KB
  return *table ? need : (size_t)BOW_MAX_FEATURES * 12;
}

int launch_bowdb_query(const BowQueryArgs& a, int Q, hipStream_t st) {
  if (Q < 1 || a.N < 1) return 0;
  bool table = false;
  const size_t lds = bowdb_query_lds(a.n_words, &table);
  auto kern = table ? bowdb_query_kernel<true> : bowdb_query_kernel<false>;
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 1;
  const dim3 grid(Q, (a.N + a.frames_per_wg - 1) / a.frames_per_wg);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
  return 0;
}

void launch_bowdb_select(const BowSelectArgs& a, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(bowdb_select_kernel, dim3(Q), dim3(256), 0, st, a);
}

void launch_bowdb_topk(const BowTopkArgs& a, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(bowdb_topk_kernel, dim3(Q), dim3(64), 0, st, a);
}

void launch_bowdb_gather(const BowGatherArgs& a, int pairs, hipStream_t st) {
  if (pairs < 1) return;
  hipLaunchKernelGGL(bowdb_gather_kernel, dim3(pairs), dim3(256), 0, st, a);
}

void launch_bowdb_best(const BowBestArgs& a, int Q, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(bowdb_best_kernel, dim3(Q), dim3(256), 0, st, a);
}

}  // namespace airfe
