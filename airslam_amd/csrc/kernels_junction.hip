// airfe — relocalisation's junction term (src/frame.cc:581-629, src/map_user.cc:285-331) as sparse integer counts.  Contract: include/airfe.h
// ("Junction term"); the statement the lanes call: junction_core.h.  The only floating-point operations are jn_extra's (one division, one add, one
// multiply on the score of the unchanged bowdb_query_kernel); the file is compiled with -ffp-contract=off.
//   junction_connect_kernel  (frame)  the junctions' pixels in LDS, a thread per line scans them for both endpoints; the directed edges are merged into a
//                            sorted distinct list in LDS, a chunk of lines at a time (bitonic sort + order-preserving compaction)
//   junction_keys_kernel     (frame)  the word table (word, cnt, conn) and the key table (word[a] << 32 | word[b], multiplicity) of one frame
//   junction_term_kernel     (query, slice of frames)  the query's two tables in LDS; a wave takes one stored frame at a time, its lanes stride over the
//                            frame's tables and binary-search the query's; integer partial sums reduced across the wave
#include "common.h"
#include "kernels.h"
#include "junction_core.h"
#include "wg_prims.h"

namespace airfe {

namespace {

#define JN_MERGE 8192                 // the connect kernel's merge buffer: the kept edges + the chunk's candidates

__device__ __forceinline__ int jn_pow2(int n) {
  int P = 256;
  while (P < n) P <<= 1;
  return P;
}

__global__ __launch_bounds__(256) void junction_connect_kernel(JunctionConnectArgs a) {
  __shared__ int px[JN_MAX_JUNCTIONS], py[JN_MAX_JUNCTIONS];
  __shared__ unsigned buf[JN_MERGE];
  __shared__ unsigned uniq[JN_MAX_EDGES];
  __shared__ int scan[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nj = clamp_count(a.njunc[b], a.capJ), nl = clamp_count(a.nlines[b], a.capL);
  const float* junc = a.junc + (size_t)b * a.capJ * 259;
  const double* lines = a.lines + (size_t)b * a.capL * 4;
  int32_t* pair = a.line_pair ? a.line_pair + (size_t)b * a.capL * 2 : nullptr;
  for (int i = t; i < nj; i += 256) jn_pixel(junc + (size_t)i * 259, a.W, a.H, &px[i], &py[i]);
  __syncthreads();
  int cnt = 0;                                                // kept distinct edges: buf[0 .. cnt), ascending (the same value in every thread)
  bool over = false;
  for (int l0 = 0; l0 < nl;) {
    const int chunk = min((JN_MERGE - cnt) / 2, nl - l0);     // cnt <= ecap <= 4096: at least 2048 lines per round
    for (int i = t; i < chunk; i += 256) {
      const double* p = lines + (size_t)(l0 + i) * 4;
      int ja = jn_match(px, py, nj, p[0], p[1]);
      int jb = ja < 0 ? -1 : jn_match(px, py, nj, p[2], p[3]);        // frame.cc:621: the second end is not looked at without the first
      if (jb < 0) ja = -1;
      if (pair) { pair[2 * (l0 + i)] = ja; pair[2 * (l0 + i) + 1] = jb; }
      if (!over) {
        buf[cnt + 2 * i] = ja < 0 ? 0xFFFFFFFFu : jn_edge_key(ja, jb);
        buf[cnt + 2 * i + 1] = ja < 0 ? 0xFFFFFFFFu : jn_edge_key(jb, ja);
      }
    }
    l0 += chunk;
    if (over) continue;
    const int total = cnt + 2 * chunk, P = jn_pow2(total), per = P / 256;
    for (int i = total + t; i < P; i += 256) buf[i] = 0xFFFFFFFFu;
    block_sort_asc<256>(buf, P);
    int heads = 0;                                            // thread t owns positions per t .. per t + per - 1
    for (int p = per * t; p < per * t + per; ++p) {
      const unsigned k = buf[p];
      if (k != 0xFFFFFFFFu && (p == 0 || buf[p - 1] != k)) ++heads;
    }
    int nu = 0;
    int slot = block_excl_scan<256>(heads, scan, &nu);
    if (nu > a.ecap) { over = true; cnt = 0; continue; }      // (nu is the same in every thread)
    for (int p = per * t; p < per * t + per; ++p) {
      const unsigned k = buf[p];
      if (k != 0xFFFFFFFFu && (p == 0 || buf[p - 1] != k)) uniq[slot++] = k;
    }
    __syncthreads();
    for (int i = t; i < nu; i += 256) buf[i] = uniq[i];
    cnt = nu;
    __syncthreads();
  }
  int32_t* edge = a.edge + (size_t)b * a.ecap * 2;
  for (int i = t; i < cnt; i += 256) {
    edge[2 * i] = (int32_t)(buf[i] >> 16);
    edge[2 * i + 1] = (int32_t)(buf[i] & 0xFFFFu);
  }
  if (t == 0) {
    a.nedge[b] = cnt;
    a.status[b] = over ? JN_OVERFLOW : JN_OK;
  }
}

__global__ __launch_bounds__(256) void junction_keys_kernel(JunctionKeysArgs a) {
  __shared__ unsigned long long key[JN_MAX_EDGES];
  __shared__ int hp[JN_MAX_EDGES + 1];
  __shared__ unsigned wd[JN_MAX_JUNCTIONS];
  __shared__ int conn[JN_MAX_JUNCTIONS];
  __shared__ int scan[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const size_t f = (size_t)a.first + b;
  const bool bad = a.status_in && a.status_in[b] != JN_OK;
  const int nj = clamp_count(a.nj[b], a.cap), ne = bad ? 0 : clamp_count(a.nedge[b], a.ecap);
  const unsigned* word = a.word + (size_t)b * a.cap;
  const int32_t* edge = a.edge + (size_t)b * a.ecap * 2;
  if (a.out_word)
    for (int i = t; i < nj; i += 256) a.out_word[f * a.cap + i] = word[i];
  if (t == 0) {
    if (a.out_nj) a.out_nj[f] = nj;
    a.status[f] = bad ? JN_OVERFLOW : JN_OK;
  }
  if (bad) {
    if (t == 0) { a.nuw[f] = 0; a.nuk[f] = 0; }
    return;
  }
  for (int i = t; i < nj; i += 256) { wd[i] = word[i]; conn[i] = 0; }
  __syncthreads();
  // the key table; conn[a] = 1 for every junction with an edge (every writer stores the same value)
  const int PK = jn_pow2(ne);
  for (int e = t; e < PK; e += 256) {
    unsigned long long k = ~0ull;
    if (e < ne) {
      const int ja = edge[2 * e], jb = edge[2 * e + 1];
      if (jn_edge_ok(ja, jb, nj)) {
        conn[ja] = 1;
        if (wd[ja] != JN_NO_WORD && wd[jb] != JN_NO_WORD) k = jn_word_key(wd[ja], wd[jb]);
      }
    }
    key[e] = k;
  }
  block_sort_asc<256>(key, PK);
  {
    const int per = PK / 256;
    int heads = 0, valid = 0;
    for (int p = per * t; p < per * t + per; ++p) {
      const unsigned long long k = key[p];
      if (k == ~0ull) break;
      ++valid;
      if (p == 0 || key[p - 1] != k) ++heads;
    }
    int nu = 0;
    int slot = block_excl_scan<256>(heads, scan, &nu);
    const int nv = block_sum<256>(valid, scan);
    for (int p = per * t; p < per * t + per; ++p) {
      const unsigned long long k = key[p];
      if (k == ~0ull) break;
      if (p == 0 || key[p - 1] != k) hp[slot++] = p;
    }
    if (t == 0) { hp[nu] = nv; a.nuk[f] = nu; }
    __syncthreads();
    for (int i = t; i < nu; i += 256) {
      a.ukey[f * a.ecap + i] = key[hp[i]];
      a.kcnt[f * a.ecap + i] = hp[i + 1] - hp[i];
    }
    __syncthreads();
  }
  // the word table: (word, junction) keys sorted; the thread that owns a segment's head walks the segment
  const int PW = jn_pow2(nj);
  for (int i = t; i < PW; i += 256) key[i] = i < nj && wd[i] != JN_NO_WORD ? jn_word_key(wd[i], (unsigned)i) : ~0ull;
  block_sort_asc<256>(key, PW);
  const int per = PW / 256;
  int heads = 0;
  for (int p = per * t; p < per * t + per; ++p) {
    const unsigned long long k = key[p];
    if (k != ~0ull && (p == 0 || (unsigned)(key[p - 1] >> 32) != (unsigned)(k >> 32))) ++heads;
  }
  int nu = 0;
  int slot = block_excl_scan<256>(heads, scan, &nu);
  for (int p = per * t; p < per * t + per; ++p) {
    const unsigned long long k = key[p];
    if (k == ~0ull) break;
    const unsigned w = (unsigned)(k >> 32);
    if (p != 0 && (unsigned)(key[p - 1] >> 32) == w) continue;
    int c = 0, cc = 0;
    for (int q = p; q < PW && (unsigned)(key[q] >> 32) == w && key[q] != ~0ull; ++q) { ++c; cc += conn[(unsigned)key[q]]; }
    a.uword[f * a.cap + slot] = w;
    a.wcnt[f * a.cap + slot] = c;
    a.wconn[f * a.cap + slot] = cc;
    ++slot;
  }
  if (t == 0) a.nuw[f] = nu;
}

__global__ __launch_bounds__(256) void junction_term_kernel(JunctionTermArgs a) {
  __shared__ unsigned long long q_ukey[JN_MAX_EDGES];
  __shared__ int q_kcnt[JN_MAX_EDGES];
  __shared__ unsigned q_uword[JN_MAX_JUNCTIONS];
  __shared__ int q_wconn[JN_MAX_JUNCTIONS];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool q_ok = a.q_status[q] == JN_OK;
  const int q_nuw = q_ok ? clamp_count(a.q_nuw[q], a.cap) : 0, q_nuk = q_ok ? clamp_count(a.q_nuk[q], a.ecap) : 0;
  for (int i = t; i < q_nuw; i += 256) {
    q_uword[i] = a.q_uword[(size_t)q * a.cap + i];
    q_wconn[i] = a.q_wconn[(size_t)q * a.cap + i];
  }
  for (int i = t; i < q_nuk; i += 256) {
    q_ukey[i] = a.q_ukey[(size_t)q * a.ecap + i];
    q_kcnt[i] = a.q_kcnt[(size_t)q * a.ecap + i];
  }
  __syncthreads();
  const int f0 = blockIdx.y * a.frames_per_wg, f1 = min(a.N, f0 + a.frames_per_wg);
  for (int f = f0 + wave; f < f1; f += 4) {
    const bool ok = q_ok && a.f_status[f] == JN_OK;
    int mn = 0, lmn = 0;
    if (ok) {
      const int nuw = clamp_count(a.f_nuw[f], a.cap), nuk = clamp_count(a.f_nuk[f], a.ecap);
      const unsigned* uw = a.f_uword + (size_t)f * a.cap;
      const int* wc = a.f_wcnt + (size_t)f * a.cap;
      for (int e = lane; e < nuw; e += 64) {
        const int s = jn_find(q_uword, q_nuw, uw[e]);
        if (s >= 0) mn += q_wconn[s] * wc[e];
      }
      const unsigned long long* uk = a.f_ukey + (size_t)f * a.ecap;
      const int* kc = a.f_kcnt + (size_t)f * a.ecap;
      for (int e = lane; e < nuk; e += 64) {
        const int s = jn_find(q_ukey, q_nuk, uk[e]);
        if (s >= 0) lmn += q_kcnt[s] * kc[e];
      }
    }
    mn = wave_sum(mn);
    lmn = wave_sum(lmn);
    if (lane == 0) {
      const size_t o = (size_t)q * a.N + f;
      a.extra[o] = ok ? jn_extra(a.score[o], mn, lmn) : 0.0;
      if (a.match_num) a.match_num[o] = mn;
      if (a.line_match_num) a.line_match_num[o] = lmn;
    }
  }
}

}  // namespace

void launch_junction_connect(const JunctionConnectArgs& a, int B, hipStream_t st) {
  if (B < 1) return;
  hipLaunchKernelGGL(junction_connect_kernel, dim3(B), dim3(256), 0, st, a);
}

void launch_junction_keys(const JunctionKeysArgs& a, int B, hipStream_t st) {
  if (B < 1) return;
  hipLaunchKernelGGL(junction_keys_kernel, dim3(B), dim3(256), 0, st, a);
}

void launch_junction_term(const JunctionTermArgs& a, int Q, hipStream_t st) {
  if (Q < 1 || a.N < 1) return;
  const dim3 grid(Q, (a.N + a.frames_per_wg - 1) / a.frames_per_wg);
  hipLaunchKernelGGL(junction_term_kernel, grid, dim3(256), 0, st, a);
}

}  // namespace airfe
