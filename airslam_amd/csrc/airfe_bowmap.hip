// airfe — the database's map side beyond its tables (include/airfe.h "Map-point ids and the covisibility build", "Map-point triangulation", "Map-point merge"): the
// id table, the covisibility build, the map-point triangulation with its host statement and the map-point merge (kernels_covis.hip, kernels_triangulate.hip,
// kernels_merge.hip).
#include "airfe_bowdb.h"
#include "covis_core.h"
#include "merge_core.h"
#include "triangulate_core.h"

extern "C" {

/* ---- map-point ids and the covisibility build (include/airfe.h "Map-point ids and the covisibility build"; kernels_covis.hip, covis_core.h) ------- */
// the build's work arrays inside c_scratch: sized by the database and max_points alone, so the block reserved at attach is never replaced by a build
struct CovisWork {
  Carve k;
  size_t o_count, o_start, o_tile, o_packed, o_seg, o_rowcnt, o_info, zero_bytes;
  CovisWork(const airfe_bowdb* db, int max_points) {
    const size_t rows = (size_t)db->max_frames * db->cap, pts = (size_t)max_points + 1;
    zero_bytes = (pts + 4) * 4;                                                          // count [max_points + 1], then valid / ignored / status
    o_count = k.take(zero_bytes); o_start = k.take(pts * 4); o_tile = k.take(((pts + CV_SCAN_TILE - 1) / CV_SCAN_TILE) * 4);
    o_packed = k.take(rows * 4); o_seg = k.take(rows * 4); o_rowcnt = k.take((size_t)db->max_frames * 4); o_info = k.take(16);
  }
  // what the build and the triangulation's segments both read and write (after into())
  CovisArgs args(const airfe_bowdb* db) const {
    CovisArgs a;
    a.point_id = db->point_id; a.n = db->n; a.size = db->size; a.max_frames = db->max_frames; a.cap = db->cap; a.max_points = db->max_points;
    a.count = k.i(o_count); a.acc = a.count + (size_t)db->max_points + 1; a.start = k.i(o_start); a.tile = k.i(o_tile); a.packed = k.i(o_packed);
    return a;
  }
};

static int covis_build_queue(airfe_bowdb* db, int32_t* d_info, hipStream_t st, const char* who, int32_t** own_info) {
  airfe_ctx* c = db->c;
  if (!db->point_id) return fail(c, std::string(who) + ": no id table (airfe_bowdb_attach_point_ids)");
  if (db->size > CV_MAX_FRAMES) return fail(c, std::string(who) + ": more than 4096 frames in the database");
  CovisWork w(db, db->max_points);
  if (w.k.into(c, db->c_scratch, st)) return 1;
  if (own_info) *own_info = d_info = w.k.at<int32_t>(w.o_info);
  CovisArgs a = w.args(db);
  a.max_edges = db->max_edges; a.seg = w.k.i(w.o_seg); a.rowcnt = w.k.i(w.o_rowcnt);
  a.row_ptr = db->cov_row; a.nbr = db->cov_nbr; a.weight = db->cov_weight; a.info = d_info;
  HIPCHK(c, hipMemsetAsync(a.count, 0, w.zero_bytes, st));
  launch_covis_build(a, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// rows first_frame .. first_frame + B - 1 of the id table; ids from the host are range-checked first, behind the accessor's own checks of the table and the rows
static int point_ids_copy(airfe_bowdb* db, int first_frame, int B, const int32_t* src, int32_t* dst, hipMemcpyKind kind, hipStream_t st, const char* who) {
  if (src && kind == hipMemcpyHostToDevice && db->point_id && first_frame >= 0 && B >= 1 && B <= db->max_frames - first_frame)
    for (size_t i = 0, n = (size_t)B * db->cap; i < n; ++i)
      if (src[i] < -1 || src[i] >= db->max_points) return fail(db->c, std::string(who) + ": an id is < -1 or >= max_points (nothing was changed)");
  return table_rows_copy(db, db->point_id, "id table (airfe_bowdb_attach_point_ids)", (size_t)db->cap, first_frame, B, src, dst, kind, st, who);
}
int airfe_bowdb_attach_point_ids(airfe_bowdb* db, int max_points) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->has_map) return fail(c, "bowdb_attach_point_ids: no map state (airfe_bowdb_attach_map)");
  if (db->point_id) return fail(c, "bowdb_attach_point_ids: the id table is attached already");
  if (max_points < 1 || max_points > CV_MAX_POINTS) return fail(c, "bowdb_attach_point_ids: max_points must be 1 .. 16777216");
  const size_t rows = (size_t)db->max_frames * db->cap;
  CovisWork w(db, max_points);
  Carve k;
  const size_t o_id = k.take(rows * 4);
  if (k.into(c, db->id_table, c->stream)) return 1;
  AttachGuard guard{c, &db->id_table};
  if (w.k.into(c, db->c_scratch, c->stream) || hipMemsetAsync(k.i(o_id), 0xFF, rows * 4, c->stream) != hipSuccess ||      // every byte 0xFF: -1 in every slot
      hipStreamSynchronize(c->stream) != hipSuccess)
    return fail(c, "bowdb_attach_point_ids: out of device memory");
  guard.keep();
  db->point_id = k.i(o_id);
  db->max_points = max_points;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_point_ids_dev(airfe_bowdb* db, int first_frame, int B, const int32_t* d_ids, void* stream) try {
  BOWDB_ENTER(db);
  return point_ids_copy(db, first_frame, B, d_ids, nullptr, hipMemcpyDeviceToDevice, stream_of(db->c, stream), "bowdb_set_point_ids_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_point_ids(airfe_bowdb* db, int first_frame, int B, const int32_t* ids) try {
  BOWDB_ENTER(db);
  return point_ids_copy(db, first_frame, B, ids, nullptr, hipMemcpyHostToDevice, db->c->stream, "bowdb_set_point_ids");
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_point_ids(airfe_bowdb* db, int first_frame, int B, int32_t* ids) try {
  BOWDB_ENTER(db);
  return point_ids_copy(db, first_frame, B, nullptr, ids, hipMemcpyDeviceToHost, db->c->stream, "bowdb_get_point_ids");
} AIRFE_CATCH(db->c)

int airfe_bowdb_build_covisibility_dev(airfe_bowdb* db, int32_t* d_info, void* stream) try {
  BOWDB_ENTER(db);
  if (!d_info) return fail(db->c, "bowdb_build_covisibility_dev: bad argument");
  return covis_build_queue(db, d_info, stream_of(db->c, stream), "bowdb_build_covisibility_dev", nullptr);
} AIRFE_CATCH(db->c)

int airfe_bowdb_build_covisibility(airfe_bowdb* db, int* n_edges) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!n_edges) return fail(c, "bowdb_build_covisibility: bad argument");
  int32_t* d_info = nullptr;
  int32_t info[4] = {0, 0, 0, 0};
  if (covis_build_queue(db, nullptr, c->stream, "bowdb_build_covisibility", &d_info)) return 1;
  HIPCHK(c, hipMemcpyAsync(info, d_info, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_edges = info[1];
  if (info[0]) return fail(c, "bowdb_build_covisibility: more entries than max_edges (the graph is empty now)");
  return 0;
} AIRFE_CATCH(db->c)

/* ---- map-point triangulation (include/airfe.h "Map-point triangulation"; kernels_triangulate.hip, triangulate_core.h) ------------------------------ */
// the triangulation's own arrays inside t_scratch, sized by the database and max_points alone: the segments as filled and sorted, and the host form's
// device outputs.  The marks and the segment starts are the covisibility build's work arrays (c_scratch), rewritten by either build.
struct TriWork {
  Carve k;
  size_t o_seg, o_sorted, o_xyz, o_status, o_nobs, o_info;
  TriWork(const airfe_bowdb* db) {
    const size_t rows = (size_t)db->max_frames * db->cap, pts = (size_t)db->max_points;
    o_seg = k.take(rows * 4); o_sorted = k.take(rows * 4); o_xyz = k.take(pts * 24); o_status = k.take(pts * 4); o_nobs = k.take(pts * 4); o_info = k.take(16);
  }
};

static int triangulate_queue(airfe_bowdb* db, const double* cam, int min_observers, double* d_xyz, int32_t* d_status, int32_t* d_nobs, int32_t* d_info,
                             hipStream_t st, const char* who) {
  airfe_ctx* c = db->c;
  if (!db->has_tri) return fail(c, std::string(who) + ": no triangulation attached (airfe_bowdb_attach_triangulation)");
  if (db->size > TR_MAX_FRAMES) return fail(c, std::string(who) + ": more than 4096 frames in the database");
  if (!cam || !d_xyz || !d_status || !d_nobs || !d_info) return fail(c, std::string(who) + ": bad argument");
  TriangulateArgs t;
  if (!tr_cam(cam, t.cami)) return fail(c, std::string(who) + ": fx and fy must be finite and not zero");
  CovisWork w(db, db->max_points);
  TriWork tw(db);
  if (w.k.into(c, db->c_scratch, st) || tw.k.into(c, db->t_scratch, st)) return 1;      // (reserved at attach: neither block is replaced here)
  const CovisArgs a = w.args(db);
  t.feat = db->feat; t.n = db->n; t.pose = db->pose; t.size = db->size; t.cap = db->cap; t.feat_dim = AIRFE_FEAT_DIM; t.max_points = db->max_points;
  t.min_observers = min_observers;
  t.packed = a.packed; t.start = a.start; t.count = a.count; t.seg = tw.k.i(tw.o_seg); t.sorted = tw.k.i(tw.o_sorted);
  t.xyz = d_xyz; t.status = d_status; t.nobs = d_nobs; t.info = d_info;
  HIPCHK(c, hipMemsetAsync(a.count, 0, w.zero_bytes, st));
  HIPCHK(c, hipMemsetAsync(d_info, 0, 16, st));
  if (db->size > 0) launch_covis_segments(a, st);
  launch_triangulate(t, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

static int fill_points_queue(airfe_bowdb* db, const double* d_xyz, const int32_t* d_status, int only_missing, int32_t* d_written, hipStream_t st,
                             const char* who) {
  airfe_ctx* c = db->c;
  if (!db->has_tri) return fail(c, std::string(who) + ": no triangulation attached (airfe_bowdb_attach_triangulation)");
  if (db->size > TR_MAX_FRAMES) return fail(c, std::string(who) + ": more than 4096 frames in the database");
  if (!d_xyz || !d_status || !d_written) return fail(c, std::string(who) + ": bad argument");
  FillPointsArgs f;
  f.point_id = db->point_id; f.n = db->n; f.size = db->size; f.cap = db->cap; f.max_points = db->max_points; f.only_missing = only_missing != 0;
  f.xyz = d_xyz; f.status = d_status; f.points = db->xyz; f.written = d_written;
  HIPCHK(c, hipMemsetAsync(d_written, 0, 4, st));
  launch_fill_points(f, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_attach_triangulation(airfe_bowdb* db) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->point_id) return fail(c, "bowdb_attach_triangulation: no id table (airfe_bowdb_attach_point_ids)");
  if (db->has_tri) return fail(c, "bowdb_attach_triangulation: the triangulation is attached already");
  TriWork tw(db);
  if (tw.k.into(c, db->t_scratch, c->stream)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->has_tri = 1;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_triangulate_points_dev(airfe_bowdb* db, const double* cam, int min_observers, double* d_xyz, int32_t* d_status, int32_t* d_nobs,
                                       int32_t* d_info, void* stream) try {
  BOWDB_ENTER(db);
  return triangulate_queue(db, cam, min_observers, d_xyz, d_status, d_nobs, d_info, stream_of(db->c, stream), "bowdb_triangulate_points_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_triangulate_points(airfe_bowdb* db, const double* cam, int min_observers, double* xyz, int32_t* status, int32_t* nobs, int* n_ok) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->has_tri) return fail(c, "bowdb_triangulate_points: no triangulation attached (airfe_bowdb_attach_triangulation)");
  if (!xyz || !status || !nobs || !n_ok) return fail(c, "bowdb_triangulate_points: bad argument");
  TriWork tw(db);
  if (tw.k.into(c, db->t_scratch, c->stream)) return 1;
  int32_t info[4] = {0, 0, 0, 0};
  if (triangulate_queue(db, cam, min_observers, tw.k.d(tw.o_xyz), tw.k.at<int32_t>(tw.o_status), tw.k.at<int32_t>(tw.o_nobs), tw.k.at<int32_t>(tw.o_info),
                        c->stream, "bowdb_triangulate_points"))
    return 1;
  const size_t P = (size_t)db->max_points;
  HIPCHK(c, hipMemcpyAsync(xyz, tw.k.d(tw.o_xyz), P * 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(status, tw.k.at<int32_t>(tw.o_status), P * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(nobs, tw.k.at<int32_t>(tw.o_nobs), P * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info, tw.k.at<int32_t>(tw.o_info), 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_ok = info[0];
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_fill_points_dev(airfe_bowdb* db, const double* d_xyz, const int32_t* d_status, int only_missing, int32_t* d_written, void* stream) try {
  BOWDB_ENTER(db);
  return fill_points_queue(db, d_xyz, d_status, only_missing, d_written, stream_of(db->c, stream), "bowdb_fill_points_dev");
} AIRFE_CATCH(db->c)

int airfe_triangulate_point(const double* cam, const double* Twc, const float* xy, int n, double* xyz, int* status) try {
  double cami[4];
  if (!cam || !xyz || !status || n < 0 || (n > 0 && (!Twc || !xy))) return fail(nullptr, "triangulate_point: bad argument");
  if (!tr_cam(cam, cami)) return fail(nullptr, "triangulate_point: fx and fy must be finite and not zero");
  *status = triangulate_point_core(cami, Twc, xy, n, 2, xyz);      // (compiled beside the kernels, without contraction)
  return 0;
} AIRFE_CATCH(nullptr)

/* ---- map-point merge (include/airfe.h "Map-point merge"; kernels_merge.hip, merge_core.h) ----------------------------------------------------------- */
// the merge's arrays inside g_scratch, sized by the database and max_points alone: per point, the staging per feature row, the host form's device outputs
struct MergeCarve {
  Carve k;
  size_t o_parent, o_flags, o_src, o_best, o_root, o_staged, o_map, o_info;
  MergeCarve(const airfe_bowdb* db) {
    const size_t rows = (size_t)db->max_frames * db->cap, pts = (size_t)db->max_points;
    o_parent = k.take(pts * 4); o_flags = k.take(pts * 4); o_src = k.take(pts * 4); o_best = k.take(pts * 4); o_root = k.take(pts * 4);
    o_staged = k.take(rows * 4); o_map = k.take(pts * 4); o_info = k.take(MG_INFO * 4);
  }
  MergeWork work(const airfe_bowdb* db, int32_t* d_map, int32_t* d_info) const {
    return MergeWork{k.i(o_parent), k.i(o_flags), k.i(o_src), k.i(o_best), k.i(o_root), k.i(o_staged), db->max_frames, d_map, d_info};
  }
};

// l == nullptr: the pair form on d_pairs [P][2]
static int merge_queue(airfe_bowdb* db, const MergeLoop* l, const int32_t* d_pairs, int P, int32_t* d_map, int32_t* d_info, hipStream_t st, const char* who) {
  airfe_ctx* c = db->c;
  if (!db->has_merge) return fail(c, std::string(who) + ": no merge attached (airfe_bowdb_attach_merge)");
  if (db->size > MG_MAX_FRAMES) return fail(c, std::string(who) + ": more than 4096 frames in the database");
  if (!d_map || !d_info) return fail(c, std::string(who) + ": bad argument");
  if (l) {
    if (l->Q < 0 || l->Q > MG_MAX_QUERIES) return fail(c, std::string(who) + ": Q must be 0 .. 4096");
    if (l->mcap < 1 || l->mcap > MG_MAX_MATCHES) return fail(c, std::string(who) + ": mcap must be 1 .. 1024");
    if (l->Q > 0 && (!l->qframe || !l->stage || !l->loop || !l->Rlq || !l->tlq || !l->mask || !l->idx || !l->nmatch)) return fail(c, std::string(who) + ": bad argument");
    if (!mg_cam_ok(l->cam)) return fail(c, std::string(who) + ": fx and fy must be finite and not zero");
  }
  if (!l && (P < 0 || (P > 0 && !d_pairs))) return fail(c, std::string(who) + ": bad argument");
  MergeCarve m(db);
  if (m.k.into(c, db->g_scratch, st)) return 1;                     // (reserved at attach: the block is not replaced here)
  const MergeWork w = m.work(db, d_map, d_info);
  const MergeTables t{db->point_id, db->xyz, db->feat, db->n, db->size, db->cap, AIRFE_FEAT_DIM, db->max_points};
  HIPCHK(c, hipMemsetAsync(d_info, 0, MG_INFO * 4, st));
  if (l) launch_merge_loop(t, *l, w, st);
  else launch_merge_pairs(t, d_pairs, P, w, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_attach_merge(airfe_bowdb* db) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->point_id) return fail(c, "bowdb_attach_merge: no id table (airfe_bowdb_attach_point_ids)");
  if (db->has_merge) return fail(c, "bowdb_attach_merge: the merge is attached already");
  MergeCarve m(db);
  if (m.k.into(c, db->g_scratch, c->stream)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->has_merge = 1;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_merge_points_dev(airfe_bowdb* db, const int32_t* d_pairs, int P, int32_t* d_map, int32_t* d_info, void* stream) try {
  BOWDB_ENTER(db);
  return merge_queue(db, nullptr, d_pairs, P, d_map, d_info, stream_of(db->c, stream), "bowdb_merge_points_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_merge_points(airfe_bowdb* db, const int32_t* pairs, int P, int32_t* map, int32_t* info) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->has_merge) return fail(c, "bowdb_merge_points: no merge attached (airfe_bowdb_attach_merge)");
  if (!map || !info || P < 0 || (P > 0 && !pairs)) return fail(c, "bowdb_merge_points: bad argument");
  MergeCarve m(db);
  if (m.k.into(c, db->g_scratch, c->stream)) return 1;
  if (P > 0 && reserve(c, db->g_pairs, (size_t)P * 8, c->stream)) return 1;      // the pair list's device copy: the one block of the merge that grows with a call
  if (P > 0) HIPCHK(c, hipMemcpyAsync(db->g_pairs.p, pairs, (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
  if (merge_queue(db, nullptr, db->g_pairs.at<int32_t>(0), P, m.k.at<int32_t>(m.o_map), m.k.at<int32_t>(m.o_info), c->stream, "bowdb_merge_points")) return 1;
  HIPCHK(c, hipMemcpyAsync(map, m.k.at<int32_t>(m.o_map), (size_t)db->max_points * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info, m.k.at<int32_t>(m.o_info), MG_INFO * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_loop_merge_batch_dev(airfe_bowdb* db, const double* cam, const int32_t* d_qframe, int Q, const int* d_stage, const int32_t* d_loop,
                                     const double* d_Rlq, const double* d_tlq, const uint8_t* d_mask, const int32_t* d_idx, int mcap, const int* d_nmatch,
                                     int32_t* d_map, int32_t* d_info, void* stream) try {
  BOWDB_ENTER(db);
  if (!cam) return fail(db->c, "bowdb_loop_merge_batch_dev: bad argument");
  const MergeLoop l{d_qframe, Q, d_stage, d_loop, d_Rlq, d_tlq, d_mask, d_idx, mcap, d_nmatch, {cam[0], cam[1], cam[2], cam[3]}};
  return merge_queue(db, &l, nullptr, 0, d_map, d_info, stream_of(db->c, stream), "bowdb_loop_merge_batch_dev");
} AIRFE_CATCH(db->c)

}  // extern "C"
