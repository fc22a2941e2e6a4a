// airfe — the map-point merge of loop closure on the device: the tail of MapRefiner::RelativatePoseEstimation and MergeMappoints / MergeMappointGroup
// (src/map_refiner.cc:338-372, :409-459, :603-713).  Contract: include/airfe.h ("Map-point merge").  The rules are merge_core.h's, shared with the host
// statement.  What the atomics below decide is a minimum (the staged id, src, the best), an OR of flags, a count, or the union-find's forest, of which
// only each id's ROOT is read afterwards — the smallest id of its component whatever the order of the links: no output byte depends on the order in which
// an atomic landed.
//   merge_init_kernel      (point / row)  parent[m] = m, flags 0, src and best MG_NONE; staged -1
//   merge_gate_kernel<0>   (query, entry) step 1, the entry counts, the smallest B into the staging of an adopting row
//   merge_gate_kernel<1>   (query, entry) step 1 again, the unions: a pair entry links (A, B), an adopting entry links (B, staged[row]); both ids are marked
//   merge_pairs_kernel     (pair)         the pair form's unions and counts
//   merge_src_kernel       (frame, row)   src[m] = the smallest key of a valid row holding the marked id m with a position
//   merge_flatten_kernel   (point)        root[m]; the smallest triangulated id into best[root]; a root with another member is flagged; the ids removed
//   merge_map_kernel       (point)        map[m]; the groups
//   merge_relabel_kernel   (frame)        the rows' (id after adoption, group) in LDS; step 6 per row; ids and positions in place; the row counts
// THE UNION-FIND.  Every access to parent[] inside the linking launch is an agent-scope atomic: the XCDs' L2s are not coherent for plain accesses within a
// launch.  link(u, v) chases both to their roots and hangs the LARGER root under the smaller by a compare-and-swap that expects the larger to be a root
// still.  A root's parent changes once, to a smaller id, and the halving step of find only ever lowers a non-root's parent to another of its ancestors: a
// parent only decreases, so there is no cycle; a failed compare-and-swap means another lane has linked that root, so every retry follows progress made
// elsewhere and no launch can spin.  When all links are done a component has one root, its smallest id.
#include "common.h"
#include "merge_core.h"
#include "kernels.h"
#include "wg_prims.h"

namespace airfe {

namespace {

constexpr int MG_TOUCHED = 1, MG_HASCHILD = 2;

__device__ inline int mg_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int mg_find(int* parent, int u) {
  for (;;) {
    const int p = mg_load(parent + u);
    if (p == u) return u;
    const int g = mg_load(parent + p);
    if (g != p) (void)__hip_atomic_fetch_min(parent + u, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u = g;
  }
}

__device__ inline void mg_link(int* parent, int u, int v) {
  for (;;) {
    u = mg_find(parent, u);
    v = mg_find(parent, v);
    if (u == v) return;
    const int hi = u > v ? u : v, lo = u > v ? v : u;
    int expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
}

__device__ inline void mg_mark(int* flags, int m) { (void)__hip_atomic_fetch_or(flags + m, MG_TOUCHED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void merge_init_kernel(MergeWork w, int max_points, size_t rows) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g < (size_t)max_points) {
    w.parent[g] = (int)g;
    w.flags[g] = 0;
    w.src[g] = MG_NONE;
    w.best[g] = MG_NONE;
  }
  if (g < rows) w.staged[g] = -1;
}

template <int PHASE>
__global__ __launch_bounds__(256) void merge_gate_kernel(MergeTables t, MergeLoop l, MergeWork w) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int q = (int)(g / l.mcap), e = (int)(g % l.mcap);
  int kind = MG_DEAD, A = -1, B = -1, row = -1;
  if (q < l.Q && l.stage[q] == 0 && e < clamp_count(l.nmatch[q], l.mcap)) kind = mg_entry(t, l, q, e, &A, &B, &row);
  if (PHASE == 0) {
    if (kind == MG_ADOPT) atomicMin(reinterpret_cast<unsigned*>(w.staged) + row, (unsigned)B);      // -1 is the largest unsigned: the smallest B wins
    wave_count_add(kind == MG_PAIR || kind == MG_ADOPT, w.info + MG_I_LIVE);
    wave_count_add(kind == MG_OUTLIER, w.info + MG_I_OUTLIER);
    wave_count_add(kind == MG_EPIPOLAR, w.info + MG_I_EPIPOLAR);
  } else {
    if (kind == MG_ADOPT) A = w.staged[row];                       // (in range: a B of the launch before)
    if (kind == MG_PAIR || kind == MG_ADOPT) {
      mg_link(w.parent, A, B);
      mg_mark(w.flags, A);
      mg_mark(w.flags, B);
    }
  }
}

__global__ __launch_bounds__(256) void merge_pairs_kernel(const int32_t* pairs, int P, int max_points, MergeWork w) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool in = k < (size_t)P, ok = false;
  int A = -1, B = -1;
  if (in) {
    A = pairs[2 * k];
    B = pairs[2 * k + 1];
    ok = mg_valid_id(A, max_points) && mg_valid_id(B, max_points);
  }
  if (ok) {
    mg_link(w.parent, A, B);
    mg_mark(w.flags, A);
    mg_mark(w.flags, B);
  }
  wave_count_add(ok, w.info + MG_I_LIVE);
  wave_count_add(in && !ok, w.info + MG_I_OUTLIER);
}

__global__ __launch_bounds__(256) void merge_src_kernel(MergeTables t, MergeWork w) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int f = (int)(g / t.cap), i = (int)(g % t.cap);
  if (f >= t.size || i >= clamp_count(t.n[f], t.cap)) return;
  const int m = t.point_id[g];
  if (!mg_valid_id(m, t.max_points) || !(w.flags[m] & MG_TOUCHED) || is_nan(t.xyz[3 * g])) return;
  atomicMin(w.src + m, (int)g);
}

__global__ __launch_bounds__(256) void merge_flatten_kernel(MergeWork w, int max_points) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool removed = false;
  if (g < (size_t)max_points && (w.flags[g] & MG_TOUCHED)) {
    const int m = (int)g;
    int r = m;
    for (int p = w.parent[r]; p != r; p = w.parent[r]) r = p;      // a launch of its own: nothing writes parent[] here, plain loads see the links
    w.root[m] = r;
    if (w.src[m] != MG_NONE) atomicMin(w.best + r, m);
    if (r != m) {
      atomicOr(w.flags + r, MG_HASCHILD);
      removed = true;
    }
  }
  wave_count_add(removed, w.info + MG_I_REMOVED);
}

// the group of a marked id: its root when the component has another member, else -1
__device__ inline int mg_group(const MergeWork& w, int id) {
  const int fl = w.flags[id];
  if (!(fl & MG_TOUCHED)) return -1;
  const int r = w.root[id];
  return (r != id || (fl & MG_HASCHILD)) ? r : -1;
}

__device__ inline int mg_best(const MergeWork& w, int root) {
  const int b = w.best[root];
  return b != MG_NONE ? b : root;
}

__global__ __launch_bounds__(256) void merge_map_kernel(MergeWork w, int max_points) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool group = false;
  if (g < (size_t)max_points) {
    const int m = (int)g, r = mg_group(w, m);
    w.map[m] = r >= 0 ? mg_best(w, r) : m;
    group = r == m;
  }
  wave_count_add(group, w.info + MG_I_GROUPS);
}

__global__ __launch_bounds__(256) void merge_relabel_kernel(MergeTables t, MergeWork w) {
  __shared__ int ids[BOW_MAX_FEATURES];
  __shared__ int grp[BOW_MAX_FEATURES];                            // the row's group; -1: in none; -2: in none, but the row adopts
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int nf = clamp_count(t.n[f], t.cap);
  const size_t base = (size_t)f * t.cap;
  for (int i = tid; i < t.cap; i += 256) {
    int id = -1, g = -1;
    if (i < nf) {
      const int own = t.point_id[base + i];
      id = mg_row_id(own, w.staged[base + i], i, nf, t.max_points);
      if (id >= 0) {
        g = mg_group(w, id);
        if (g < 0 && id != own) g = -2;
      }
    }
    ids[i] = id;
    grp[i] = g;
  }
  __syncthreads();
  bool mine = false;
  for (int j = lane; j < t.cap; j += 64) mine = mine || grp[j] != -1;
  if (!__any(mine)) return;                                        // every wave reads all rows: the same answer in each, no barrier behind it
  for (int i0 = 0; i0 < nf; i0 += 256) {                           // (uniform)
    const int i = i0 + tid;
    int what = MG_KEEP;
    bool adopting = false;
    if (i < nf && grp[i] != -1) {
      const int id = ids[i];
      adopting = id != t.point_id[base + i];
      what = mg_row_decision(ids, grp, nf, i, grp[i] >= 0 ? mg_best(w, grp[i]) : -1);
      if (what != MG_KEEP || adopting) {
        const int now = what == MG_CLEAR ? -1 : (what == MG_BEST ? mg_best(w, grp[i]) : id);
        const int from = now >= 0 ? w.src[now] : MG_NONE;
        double x = quiet_nan(), y = quiet_nan(), z = quiet_nan();
        if (from != MG_NONE) { x = t.xyz[3 * (size_t)from]; y = t.xyz[3 * (size_t)from + 1]; z = t.xyz[3 * (size_t)from + 2]; }
        t.point_id[base + i] = now;
        t.xyz[3 * (base + i)] = x; t.xyz[3 * (base + i) + 1] = y; t.xyz[3 * (base + i) + 2] = z;
      }
    }
    wave_count_add(adopting, w.info + MG_I_ADOPTED);
    wave_count_add(what == MG_BEST, w.info + MG_I_RELABELLED);
    wave_count_add(what == MG_CLEAR, w.info + MG_I_CLEARED);
  }
}

inline unsigned blocks_of(size_t lanes) { return (unsigned)((lanes + 255) / 256); }

// steps 4 - 7 behind the unions
void merge_finish(const MergeTables& t, const MergeWork& w, hipStream_t st) {
  const unsigned pts = blocks_of((size_t)t.max_points);
  if (t.size > 0) hipLaunchKernelGGL(merge_src_kernel, dim3(blocks_of((size_t)t.size * t.cap)), dim3(256), 0, st, t, w);
  hipLaunchKernelGGL(merge_flatten_kernel, dim3(pts), dim3(256), 0, st, w, t.max_points);
  hipLaunchKernelGGL(merge_map_kernel, dim3(pts), dim3(256), 0, st, w, t.max_points);
  if (t.size > 0) hipLaunchKernelGGL(merge_relabel_kernel, dim3(t.size), dim3(256), 0, st, t, w);
}

void merge_init(const MergeTables& t, const MergeWork& w, hipStream_t st) {
  const size_t rows = (size_t)w.max_frames * t.cap, lanes = rows > (size_t)t.max_points ? rows : (size_t)t.max_points;
  hipLaunchKernelGGL(merge_init_kernel, dim3(blocks_of(lanes)), dim3(256), 0, st, w, t.max_points, rows);
}

}  // namespace

void launch_merge_loop(const MergeTables& t, const MergeLoop& l, const MergeWork& w, hipStream_t st) {
  merge_init(t, w, st);
  const size_t entries = (size_t)l.Q * l.mcap;
  if (entries > 0) {
    hipLaunchKernelGGL(merge_gate_kernel<0>, dim3(blocks_of(entries)), dim3(256), 0, st, t, l, w);
    hipLaunchKernelGGL(merge_gate_kernel<1>, dim3(blocks_of(entries)), dim3(256), 0, st, t, l, w);
  }
  merge_finish(t, w, st);
}

void launch_merge_pairs(const MergeTables& t, const int32_t* pairs, int P, const MergeWork& w, hipStream_t st) {
  merge_init(t, w, st);
  if (P > 0) hipLaunchKernelGGL(merge_pairs_kernel, dim3(blocks_of((size_t)P)), dim3(256), 0, st, pairs, P, t.max_points, w);
  merge_finish(t, w, st);
}

}  // namespace airfe
