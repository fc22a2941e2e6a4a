// airfe — the BoW side of libairfe.so (include/airfe.h): the BoW vector, the device-resident keyframe database with its queries and map tables, the grouping, and the
// relocalisation and loop detection composites (kernels_bowdb.hip, kernels_bowgroup.hip, kernels_loopdet.hip).  The id table, the covisibility build and the
// triangulation are in airfe_bowmap.hip, the junction term in airfe_junction.hip; the vocabulary itself (airfe_bow_load, airfe_bow_transform*) is loaded in airfe.hip.
#include "airfe_bowdb.h"
#include "fransac_core.h"
#include "pnp_core.h"
#include "poseopt_core.h"
#include "bowgroup_core.h"
#include "loopdet_core.h"

int bow_vector_queue(airfe_ctx* c, const float* d_feat, const int* d_n, int B, int cap, uint32_t* d_ids, double* d_vals, int* d_nw, uint32_t* d_word,
                     hipStream_t st) {
  const size_t rows = (size_t)B * cap;
  Carve k;
  const size_t o_word = k.take(rows * 4), o_wf = k.take(rows * 4), o_node = k.take(rows * 4);
  if (k.into(c, c->bv_scratch, st)) return 1;
  unsigned* word = d_word ? d_word : k.at<unsigned>(o_word);
  float* wf = k.at<float>(o_wf);
  int* node = k.i(o_node);
  ProfScope ps(c, ST_BOW, st, 0, (double)rows * 259 * 4);
  // the existing descent over every row of the batch (rows past a frame's count are descended too and ignored: the vector kernel reads n rows)
  launch_bow_transform(d_feat, AIRFE_FEAT_DIM, 3, (int)rows, c->bow_desc, c->bow_first, c->bow_nch, c->bow_word, c->bow_weight, word, wf, node, st);
  BowVecArgs a;
  a.word = word; a.node = node; a.n = d_n; a.cap = cap; a.weight = c->bow_weight_d; a.ids = d_ids; a.vals = d_vals; a.nw = d_nw;
  launch_bow_vector(a, B, st);
  note_launch(c, ST_BOW);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// Database::AddFrame: frame `size + b` = vector b.  kind = hipMemcpyDeviceToDevice (asynchronous on st) or hipMemcpyHostToDevice (synchronous)
int bowdb_add_impl(airfe_bowdb* db, const uint32_t* ids, const double* vals, const int* nw, const float* feat, const int* n, int B, int cap, hipMemcpyKind kind,
                   hipStream_t st, const char* who) {
  airfe_ctx* c = db->c;
  if (B < 1 || !ids || !vals || !nw || cap != db->cap) return fail(c, std::string(who) + ": bad argument (cap must be the database's)");
  if (db->keep && (!feat || !n)) return fail(c, std::string(who) + ": this database keeps the frames' features: d_feat / d_n are needed");
  if (B > db->max_frames - db->size) return fail(c, std::string(who) + ": the database is full (max_frames)");
  const size_t at = (size_t)db->size * cap, rows = (size_t)B * cap;
  HIPCHK(c, hipMemcpyAsync(db->ids + at, ids, rows * 4, kind, st));
  HIPCHK(c, hipMemcpyAsync(db->vals + at, vals, rows * 8, kind, st));
  HIPCHK(c, hipMemcpyAsync(db->nw + db->size, nw, (size_t)B * 4, kind, st));
  if (db->keep) {
    HIPCHK(c, hipMemcpyAsync(db->feat + at * AIRFE_FEAT_DIM, feat, rows * AIRFE_FEAT_DIM * 4, kind, st));
    HIPCHK(c, hipMemcpyAsync(db->n + db->size, n, (size_t)B * 4, kind, st));
  }
  if (kind == hipMemcpyHostToDevice) HIPCHK(c, hipStreamSynchronize(st));
  db->size += B;
  return 0;
}

int bowdb_dense_query_queue(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, int Q, int qcap, double* d_score, int32_t* d_sharing,
                            int* frames_per_wg, hipStream_t st, const char* who) {
  BowQueryArgs a;
  a.db_ids = db->ids; a.db_vals = db->vals; a.db_nw = db->nw; a.N = db->size; a.cap = db->cap;
  a.q_ids = d_ids; a.q_vals = d_vals; a.q_nw = d_nw; a.qcap = qcap; a.n_words = db->c->bow_nwords;
  a.frames_per_wg = (size_t)Q * db->size >= (size_t)64 * 1024 ? 64 : 16;
  a.score = d_score; a.sharing = d_sharing;
  if (frames_per_wg) *frames_per_wg = a.frames_per_wg;
  if (launch_bowdb_query(a, Q, st)) return fail(db->c, std::string(who) + ": the query table does not fit the workgroup's LDS");
  return 0;
}

// A query as one BoW stage: the dense score / sharing [Q][N] inside q_scratch (sharing: the caller's when it gives one), the dense query, and the caller's
// selection from them, select(score, sharing), which is one launch
template <class Select>
static int query_select_queue(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, int Q, int qcap, int32_t* d_sharing, hipStream_t st,
                              const char* who, Select select) {
  airfe_ctx* c = db->c;
  const size_t cells = (size_t)Q * std::max(db->size, 1);
  Carve k;
  const size_t o_score = k.take(cells * 8), o_sharing = k.take(cells * 4);
  if (k.into(c, db->q_scratch, st)) return 1;
  int32_t* sharing = d_sharing ? d_sharing : k.i(o_sharing);
  ProfScope ps(c, ST_BOW, st, 0, (double)Q * db->size * db->cap * 12);
  if (bowdb_dense_query_queue(db, d_ids, d_vals, d_nw, Q, qcap, k.d(o_score), sharing, nullptr, st, who)) return 1;
  select(k.d(o_score), sharing);
  note_launch(c, ST_BOW);
  HIPCHK(c, hipGetLastError());
  return 0;
}

extern "C" {

int airfe_bow_vector_batch_dev(airfe_ctx* c, const float* d_feat, const int* d_n, int B, int cap, uint32_t* d_ids, double* d_vals, int* d_nw,
                               uint32_t* d_word, void* stream) try {
  AIRFE_ENTER(c);
  if (!c->bow_nodes) return fail(c, "bow_vector_batch_dev: no vocabulary loaded (airfe_bow_load)");
  if (B < 1 || cap < 1 || !d_feat || !d_n || !d_ids || !d_vals || !d_nw) return fail(c, "bow_vector_batch_dev: bad argument");
  if (cap > BOW_MAX_FEATURES) return fail(c, "bow_vector_batch_dev: cap > 1024");
  if ((size_t)B * cap > (size_t)INT32_MAX) return fail(c, "bow_vector_batch_dev: batch too large");
  return bow_vector_queue(c, d_feat, d_n, B, cap, d_ids, d_vals, d_nw, d_word, stream_of(c, stream));
} AIRFE_CATCH(c)

int airfe_bow_vector(airfe_ctx* c, const float* feat, int n, uint32_t* ids, double* vals, int* nw, uint32_t* word_of_features) try {
  AIRFE_ENTER(c);
  if (!c->bow_nodes) return fail(c, "bow_vector: no vocabulary loaded (airfe_bow_load)");
  if (n < 0 || !nw || (n > 0 && (!feat || !ids || !vals))) return fail(c, "bow_vector: bad argument");
  if (n > BOW_MAX_FEATURES) return fail(c, "bow_vector: more than 1024 features");
  *nw = 0;
  if (n == 0) return 0;                                          // database.cc:60
  hipStream_t st = c->stream;
  Carve kc;
  const size_t o_n = kc.take(4), o_nw = kc.take(4), o_vals = kc.take((size_t)n * 8), o_feat = kc.take((size_t)n * AIRFE_FEAT_DIM * 4), o_ids = kc.take((size_t)n * 4),
               o_word = kc.take((size_t)n * 4);
  if (kc.into(c, c->bv_stage, st)) return 1;
  int *d_n = kc.i(o_n), *d_nw = kc.i(o_nw);
  double* d_vals = kc.d(o_vals);
  float* d_feat = kc.at<float>(o_feat);
  uint32_t *d_ids = kc.at<uint32_t>(o_ids), *d_word = kc.at<uint32_t>(o_word);
  DrainOnError drain{c, true};
  HIPCHK(c, hipMemcpyAsync(d_n, &n, 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_feat, feat, (size_t)n * AIRFE_FEAT_DIM * 4, hipMemcpyHostToDevice, st));
  if (bow_vector_queue(c, d_feat, d_n, 1, n, d_ids, d_vals, d_nw, d_word, st)) return 1;
  int k = 0;
  HIPCHK(c, hipMemcpyAsync(&k, d_nw, 4, hipMemcpyDeviceToHost, st));
  if (word_of_features) HIPCHK(c, hipMemcpyAsync(word_of_features, d_word, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (k > 0) {
    HIPCHK(c, hipMemcpyAsync(ids, d_ids, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(vals, d_vals, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  drain.armed = false;
  *nw = k;
  return 0;
} AIRFE_CATCH(c)

int airfe_bowdb_create(airfe_ctx* c, int max_frames, int cap, int keep_features, airfe_bowdb** out) try {
  AIRFE_ENTER(c);
  if (!out) return fail(c, "bowdb_create: null argument");
  *out = nullptr;
  if (max_frames < 1 || cap < 1) return fail(c, "bowdb_create: bad argument");
  if (cap > BOW_MAX_FEATURES) return fail(c, "bowdb_create: cap > 1024");
  if (!c->bow_nodes) return fail(c, "bowdb_create: no vocabulary loaded (airfe_bow_load): the database is sized by its word count");
  struct Guard { airfe_bowdb* p; ~Guard() { if (p) (void)airfe_bowdb_destroy(p); } } guard{new airfe_bowdb()};
  airfe_bowdb* db = guard.p;
  db->c = c; db->max_frames = max_frames; db->cap = cap; db->keep = keep_features != 0;
  const size_t rows = (size_t)max_frames * cap;
  const size_t bytes[5] = {rows * 4, rows * 8, (size_t)max_frames * 4, db->keep ? rows * AIRFE_FEAT_DIM * 4 : 0, db->keep ? (size_t)max_frames * 4 : 0};
  for (int t = 0; t < 5; ++t)
    if (reserve(c, db->tables[t], bytes[t], c->stream)) return 1;      // (0 bytes: no block, the pointer stays null)
  db->ids = db->tables[0].at<uint32_t>(0); db->vals = db->tables[1].at<double>(0); db->nw = db->tables[2].at<int>(0);
  db->feat = db->tables[3].at<float>(0); db->n = db->tables[4].at<int>(0);
  guard.p = nullptr;
  *out = db;
  return 0;
} AIRFE_CATCH(c)

int airfe_bowdb_destroy(airfe_bowdb* db) try {
  if (!db) return 0;
  if (db->c) { (void)enter_device(db->c); (void)hipDeviceSynchronize(); }
  if (db->c)
    for (DevBlock* b : {db->tables, db->tables + 1, db->tables + 2, db->tables + 3, db->tables + 4, &db->map_tables, &db->id_table, &db->q_scratch, &db->m_scratch,
                        &db->r_scratch, &db->l_scratch, &db->c_scratch, &db->t_scratch, &db->g_scratch, &db->g_pairs, &db->j_block})
      release(db->c, *b);
  delete db;
  return 0;
} AIRFE_CATCH(nullptr)

int airfe_bowdb_clear(airfe_bowdb* db) try {
  if (!db) return 1;
  db->size = 0;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_size(const airfe_bowdb* db) try {
  return db ? db->size : -1;
} AIRFE_CATCH(nullptr)

int airfe_bowdb_add_batch_dev(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, const float* d_feat, const int* d_n, int B,
                              int cap, void* stream) try {
  BOWDB_ENTER(db);
  return bowdb_add_impl(db, d_ids, d_vals, d_nw, d_feat, d_n, B, cap, hipMemcpyDeviceToDevice, stream_of(db->c, stream), "bowdb_add_batch_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_add(airfe_bowdb* db, const uint32_t* ids, const double* vals, const int* nw, const float* feat, const int* n, int B, int cap) try {
  BOWDB_ENTER(db);
  return bowdb_add_impl(db, ids, vals, nw, feat, n, B, cap, hipMemcpyHostToDevice, db->c->stream, "bowdb_add");
} AIRFE_CATCH(db->c)

// Database::Query + the sharing-word filter + Database::Score for Q device vectors on `st` (the body of airfe_bowdb_query_batch_dev; the relocalisation
// composite queues the same code)
static int bowdb_query_queue(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, int Q, int cap, const airfe_bowdb_filter* filter,
                             int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap, int* d_ncand, int* d_max_sharing,
                             int32_t* d_sharing, hipStream_t st) {
  BowSelectArgs s;
  s.N = db->size; s.ratio = filter->ratio; s.min_words = filter->min_words;
  s.max_index = filter->d_max_index; s.exclude = filter->d_exclude; s.exclude_words = filter->exclude_words;
  s.cand_frame = d_cand_frame; s.cand_sharing = d_cand_sharing; s.cand_score = d_cand_score; s.ccap = ccap; s.ncand = d_ncand; s.max_sharing = d_max_sharing;
  return query_select_queue(db, d_ids, d_vals, d_nw, Q, cap, d_sharing, st, "bowdb_query_batch_dev", [&](double* score, int32_t* sharing) {
    s.score = score; s.sharing = sharing;
    launch_bowdb_select(s, Q, st);
  });
}

int airfe_bowdb_query_batch_dev(airfe_bowdb* db, const uint32_t* d_ids, const double* d_vals, const int* d_nw, int Q, int cap,
                                const airfe_bowdb_filter* filter, int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap,
                                int* d_ncand, int* d_max_sharing, int32_t* d_sharing, void* stream) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (Q < 1 || cap < 1 || ccap < 1 || !d_ids || !d_vals || !d_nw || !filter || !d_cand_frame || !d_cand_sharing || !d_cand_score || !d_ncand || !d_max_sharing)
    return fail(c, "bowdb_query_batch_dev: bad argument");
  if (cap > BOW_MAX_FEATURES) return fail(c, "bowdb_query_batch_dev: cap > 1024");
  if (filter->d_exclude && filter->exclude_words < 1) return fail(c, "bowdb_query_batch_dev: d_exclude needs exclude_words");
  return bowdb_query_queue(db, d_ids, d_vals, d_nw, Q, cap, filter, d_cand_frame, d_cand_sharing, d_cand_score, ccap, d_ncand, d_max_sharing, d_sharing,
                           stream_of(c, stream));
} AIRFE_CATCH(db->c)

int airfe_bowdb_topk_dev(airfe_bowdb* db, const int32_t* d_cand_frame, const double* d_cand_score, const int* d_ncand, int Q, int ccap, int K,
                         int32_t* d_top, double* d_top_score, void* stream) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (Q < 1 || ccap < 1 || K < 1 || K > 8 || !d_cand_frame || !d_cand_score || !d_ncand || !d_top) return fail(c, "bowdb_topk_dev: bad argument (K = 1..8)");
  BowTopkArgs a;
  a.cand_frame = d_cand_frame; a.cand_score = d_cand_score; a.ncand = d_ncand; a.ccap = ccap; a.K = K; a.top = d_top; a.top_score = d_top_score;
  launch_bowdb_topk(a, Q, stream_of(c, stream));
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(db->c)

// the best-candidate rule around the matcher for Q queries x K candidates on `st` (the body of airfe_bowdb_match_candidates_batch_dev; the relocalisation
// composite queues the same code)
static int bowdb_match_queue(airfe_ctx* c, airfe_bowdb* db, const float* d_qfeat, const int* d_qn, int Q, int cap, const int32_t* d_cand, int K,
                             int outlier_rejection, int32_t* d_best, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch, int* d_nmatch_all,
                             hipStream_t st) {
  const int P = Q * K;
  Carve k;
  const size_t fb = (size_t)P * cap * AIRFE_FEAT_DIM * 4, cb = (size_t)P * 4;
  const size_t o_f0 = k.take(fb), o_f1 = k.take(fb), o_idx = k.take((size_t)P * mcap * 8), o_score = k.take((size_t)P * mcap * 4), o_n0 = k.take(cb),
               o_n1 = k.take(cb), o_nm = k.take(cb);
  if (k.into(c, db->m_scratch, st)) return 1;
  BowGatherArgs g;
  g.f0 = k.at<float>(o_f0); g.f1 = k.at<float>(o_f1); g.n0 = k.i(o_n0); g.n1 = k.i(o_n1);
  int32_t* p_idx = k.at<int32_t>(o_idx);
  float* p_score = k.at<float>(o_score);
  int* p_nm = k.i(o_nm);
  g.qfeat = d_qfeat; g.qn = d_qn; g.db_feat = db->feat; g.db_n = db->n; g.N = db->size; g.cap = cap; g.cand = d_cand; g.K = K;
  launch_bowdb_gather(g, P, st);
  HIPCHK(c, hipGetLastError());
  // MatchingPoints(query_features, good_candidate_features, matches, true) (map_user.cc:369): the context's own entries, called
  if (lightglue_dev(c, g.f0, g.n0, g.f1, g.n1, P, cap, AIRFE_FEAT_DIM, 1, 1, p_idx, p_score, mcap, p_nm, nullptr, st)) return 1;
  if (outlier_rejection && fransac_queue(c, g.f0, g.f1, P, cap, p_idx, p_score, mcap, p_nm, nullptr, st)) return 1;
  BowBestArgs b;
  b.cand = d_cand; b.K = K; b.N = db->size; b.mcap = mcap; b.idx_all = p_idx; b.score_all = p_score; b.nmatch_all = p_nm;
  b.best = d_best; b.idx = d_idx; b.score = d_score; b.nmatch = d_nmatch; b.out_nmatch_all = d_nmatch_all;
  launch_bowdb_best(b, Q, st);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_match_candidates_batch_dev(airfe_ctx* c, airfe_bowdb* db, const float* d_qfeat, const int* d_qn, int Q, int cap, const int32_t* d_cand, int K,
                                           int outlier_rejection, int32_t* d_best, int32_t* d_idx, float* d_score, int mcap, int* d_nmatch,
                                           int* d_nmatch_all, void* stream) try {
  AIRFE_ENTER(c);
  if (!db || db->c != c) return fail(c, "bowdb_match_candidates_batch_dev: the database belongs to another context");
  if (Q < 1 || K < 1 || K > 5 || mcap < 1 || !d_qfeat || !d_qn || !d_cand || !d_best || !d_idx || !d_score || !d_nmatch)
    return fail(c, "bowdb_match_candidates_batch_dev: bad argument (K = 1..5)");
  if (!db->keep) return fail(c, "bowdb_match_candidates_batch_dev: the database was created without keep_features");
  if (cap != db->cap) return fail(c, "bowdb_match_candidates_batch_dev: cap must be the database's");
  if (mcap > FR_MAX_MATCHES) return fail(c, "bowdb_match_candidates_batch_dev: mcap > 1024");
  if ((long long)Q * K > c->Pmax) return fail(c, "bowdb_match_candidates_batch_dev: Q * K pairs exceed cfg.max_batch");
  return bowdb_match_queue(c, db, d_qfeat, d_qn, Q, cap, d_cand, K, outlier_rejection, d_best, d_idx, d_score, mcap, d_nmatch, d_nmatch_all, stream_of(c, stream));
} AIRFE_CATCH(c)

/* ---- map state in the database, the grouping and the relocalisation composite (include/airfe.h "Grouping", "Relocalisation composite";
 * kernels_bowgroup.hip, bowgroup_core.h) ------------------------------------------------------------------------------------------------------------ */
int airfe_bowdb_attach_map(airfe_bowdb* db, int max_edges) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (db->has_map) return fail(c, "bowdb_attach_map: the map state is attached already");
  if (!db->keep) return fail(c, "bowdb_attach_map: the database was created without keep_features");
  if (max_edges < 1) return fail(c, "bowdb_attach_map: bad argument");
  const size_t F = (size_t)db->max_frames, rows = F * db->cap, E = (size_t)max_edges;
  Carve k;
  const size_t o_xyz = k.take(rows * 24), o_row = k.take((F + 1) * 4), o_nbr = k.take(E * 4), o_weight = k.take(E * 4), o_pos = k.take(F * 24), o_pose = k.take(F * 128),
               o_ur = k.take(rows * 8);
  if (k.into(c, db->map_tables, c->stream)) return 1;
  AttachGuard guard{c, &db->map_tables};
  HIPCHK(c, hipMemsetAsync(k.d(o_xyz), 0xFF, rows * 24, c->stream));                  // every byte 0xFF: a NaN in every slot
  HIPCHK(c, hipMemsetAsync(k.i(o_row), 0, (F + 1) * 4, c->stream));                   // an empty graph
  HIPCHK(c, hipMemsetAsync(k.i(o_nbr), 0, E * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(k.i(o_weight), 0, E * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(k.d(o_pos), 0xFF, F * 24, c->stream));
  launch_loopdet_init(k.d(o_pose), k.d(o_ur), db->max_frames, db->cap, c->stream);    // identity poses, no right image anywhere
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  guard.keep();
  db->xyz = k.d(o_xyz); db->cov_row = k.i(o_row); db->cov_nbr = k.i(o_nbr); db->cov_weight = k.i(o_weight); db->pos = k.d(o_pos); db->pose = k.d(o_pose);
  db->u_right = k.d(o_ur);
  db->max_edges = max_edges;
  db->has_map = 1;
  return 0;
} AIRFE_CATCH(db->c)

// rows of one of the map state's f64 tables
static int bowdb_rows_copy(airfe_bowdb* db, double* table, size_t per, int first_frame, int B, const void* src, void* dst, hipMemcpyKind kind, hipStream_t st,
                           const char* who) {
  return table_rows_copy(db, table, "map state (airfe_bowdb_attach_map)", per, first_frame, B, src, dst, kind, st, who);
}

int airfe_bowdb_set_points_dev(airfe_bowdb* db, int first_frame, int B, const double* d_xyz, void* stream) try {
  BOWDB_ENTER(db);
  return bowdb_rows_copy(db, db->xyz, (size_t)db->cap * 3, first_frame, B, d_xyz, nullptr, hipMemcpyDeviceToDevice, stream_of(db->c, stream), "bowdb_set_points_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_points(airfe_bowdb* db, int first_frame, int B, const double* xyz) try {
  BOWDB_ENTER(db);
  return bowdb_rows_copy(db, db->xyz, (size_t)db->cap * 3, first_frame, B, xyz, nullptr, hipMemcpyHostToDevice, db->c->stream, "bowdb_set_points");
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_points(airfe_bowdb* db, int first_frame, int B, double* xyz) try {
  BOWDB_ENTER(db);
  return bowdb_rows_copy(db, db->xyz, (size_t)db->cap * 3, first_frame, B, nullptr, xyz, hipMemcpyDeviceToHost, db->c->stream, "bowdb_get_points");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_positions(airfe_bowdb* db, int first_frame, int B, const double* pos) try {
  BOWDB_ENTER(db);
  if (bowdb_rows_copy(db, db->pos, 3, first_frame, B, pos, nullptr, hipMemcpyHostToDevice, db->c->stream, "bowdb_set_positions")) return 1;
  db->has_pos = 1;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_covisibility(airfe_bowdb* db, const int32_t* row_ptr, const int32_t* nbr, const int32_t* weight, int n_frames) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->has_map) return fail(c, "bowdb_set_covisibility: no map state (airfe_bowdb_attach_map)");
  if (n_frames < 0 || n_frames > db->max_frames || !row_ptr) return fail(c, "bowdb_set_covisibility: bad argument (n_frames beyond max_frames)");
  if (row_ptr[0] != 0) return fail(c, "bowdb_set_covisibility: row_ptr[0] must be 0");
  for (int f = 0; f < n_frames; ++f)
    if (row_ptr[f + 1] < row_ptr[f]) return fail(c, "bowdb_set_covisibility: row_ptr must not decrease");
  const int E = row_ptr[n_frames];
  if (E > db->max_edges) return fail(c, "bowdb_set_covisibility: more entries than max_edges");
  if (E > 0 && (!nbr || !weight)) return fail(c, "bowdb_set_covisibility: bad argument");
  for (int f = 0; f < n_frames; ++f)
    for (int e = row_ptr[f]; e < row_ptr[f + 1]; ++e)
      if (nbr[e] < 0 || (e > row_ptr[f] && nbr[e] <= nbr[e - 1]))
        return fail(c, "bowdb_set_covisibility: every row must be strictly ascending in nbr (nothing was changed)");
  std::vector<int32_t> rows((size_t)db->max_frames + 1, E);                                // frames past n_frames: empty rows
  std::copy(row_ptr, row_ptr + n_frames + 1, rows.begin());
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(db->cov_row, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
  if (E > 0) {
    HIPCHK(c, hipMemcpyAsync(db->cov_nbr, nbr, (size_t)E * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(db->cov_weight, weight, (size_t)E * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_covisibility(airfe_bowdb* db, int32_t* row_ptr, int32_t* nbr, int32_t* weight, int edge_cap, int* n_edges) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->has_map) return fail(c, "bowdb_get_covisibility: no map state (airfe_bowdb_attach_map)");
  if (!row_ptr || !n_edges || edge_cap < 0) return fail(c, "bowdb_get_covisibility: bad argument");
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(row_ptr, db->cov_row, ((size_t)db->max_frames + 1) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int E = row_ptr[db->max_frames];
  *n_edges = E;
  if (E > edge_cap) return fail(c, "bowdb_get_covisibility: more entries than edge_cap");
  if (E > 0) {
    if (!nbr || !weight) return fail(c, "bowdb_get_covisibility: bad argument");
    HIPCHK(c, hipMemcpyAsync(nbr, db->cov_nbr, (size_t)E * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(weight, db->cov_weight, (size_t)E * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  return 0;
} AIRFE_CATCH(db->c)

// the grouping for Q candidate lists on `st`
static int bowdb_group_queue(airfe_bowdb* db, int mode, const int32_t* d_cand_frame, const double* d_cand_score, const int* d_ncand, int Q, int ccap, int K,
                             const double* d_extra, const double* d_qpos, const double* d_max_dist, int32_t* d_group_frame, double* d_group_score,
                             int* d_ngroups, int* d_status, hipStream_t st) {
  airfe_ctx* c = db->c;
  BowGroupArgs a;
  a.mode = mode; a.cand_frame = d_cand_frame; a.cand_score = d_cand_score; a.ncand = d_ncand; a.ccap = ccap; a.K = K;
  a.row_ptr = db->cov_row; a.nbr = db->cov_nbr; a.weight = db->cov_weight; a.rows = db->max_frames;
  a.extra = d_extra; a.n_extra = db->size; a.pos = db->pos; a.pos_rows = db->max_frames; a.qpos = d_qpos; a.max_dist = d_max_dist;
  a.group_frame = d_group_frame; a.group_score = d_group_score; a.ngroups = d_ngroups; a.status = d_status;
  if (launch_bowgroup(a, Q, st)) return fail(c, "bowdb_group_dev: the candidate list does not fit the workgroup's LDS");
  HIPCHK(c, hipGetLastError());
  return 0;
}

int airfe_bowdb_group_dev(airfe_bowdb* db, int mode, const int32_t* d_cand_frame, const double* d_cand_score, const int* d_ncand, int Q, int ccap, int K,
                          const double* d_extra, const double* d_qpos, const double* d_max_dist, int32_t* d_group_frame, double* d_group_score,
                          int* d_ngroups, int* d_status, void* stream) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->has_map) return fail(c, "bowdb_group_dev: no map state (airfe_bowdb_attach_map)");
  if (Q < 1 || ccap < 1 || K < 1 || !d_cand_frame || !d_cand_score || !d_ncand || !d_group_frame || !d_group_score || !d_ngroups || !d_status)
    return fail(c, "bowdb_group_dev: bad argument");
  if (mode != BG_MODE_RELOC && mode != BG_MODE_LOOP) return fail(c, "bowdb_group_dev: mode is 0 (relocalisation) or 1 (loop detection)");
  if (K > (mode == BG_MODE_RELOC ? 3 : 5)) return fail(c, "bowdb_group_dev: K <= 3 (relocalisation) / K <= 5 (loop detection)");
  if (ccap > BG_MAX_CAND) return fail(c, "bowdb_group_dev: ccap > 4096");
  if (mode == BG_MODE_LOOP && (!d_qpos || !d_max_dist || !db->has_pos))
    return fail(c, "bowdb_group_dev: the loop form needs d_qpos, d_max_dist and the keyframe positions (airfe_bowdb_set_positions)");
  return bowdb_group_queue(db, mode, d_cand_frame, d_cand_score, d_ncand, Q, ccap, K, d_extra, d_qpos, d_max_dist, d_group_frame, d_group_score, d_ngroups,
                           d_status, stream_of(c, stream));
} AIRFE_CATCH(db->c)

int airfe_relocalize_batch_dev(airfe_ctx* c, airfe_bowdb* db, const airfe_reloc_cfg* cfg, const float* d_qfeat, const int* d_qn, int Q, int cap,
                               const double* d_extra, int* d_ok, int* d_stage, double* d_Twc, int32_t* d_best, int* d_num, uint8_t* d_mask, int32_t* d_idx,
                               float* d_score, int mcap, int* d_nmatch, int* d_pnp_count, void* stream) try {
  AIRFE_ENTER(c);
  if (!db || db->c != c) return fail(c, "relocalize_batch_dev: the database belongs to another context");
  if (!db->has_map) return fail(c, "relocalize_batch_dev: no map state (airfe_bowdb_attach_map)");
  if (!cfg || Q < 1 || mcap < 1 || !d_qfeat || !d_qn || !d_ok || !d_stage || !d_Twc || !d_best || !d_num || !d_mask || !d_idx || !d_score || !d_nmatch)
    return fail(c, "relocalize_batch_dev: bad argument");
  if (cfg->K < 1 || cfg->K > 3) return fail(c, "relocalize_batch_dev: cfg.K = 1..3");
  if (cap != db->cap) return fail(c, "relocalize_batch_dev: cap must be the database's");
  if (mcap > PNP_MAX_POINTS) return fail(c, "relocalize_batch_dev: mcap > 1024");
  if ((long long)Q * cfg->K > c->Pmax) return fail(c, "relocalize_batch_dev: Q * K pairs exceed cfg.max_batch");
  if (!c->bow_nodes) return fail(c, "relocalize_batch_dev: no vocabulary loaded (airfe_bow_load)");
  const int N = db->size, ccap = std::max(N, 1), K = cfg->K;
  if (ccap > BG_MAX_CAND) return fail(c, "relocalize_batch_dev: more than 4096 frames in the database");
  hipStream_t st = stream_of(c, stream);
  // one block, every part 256-byte aligned
  Carve k;
  const size_t qc = (size_t)Q * cap, qm = (size_t)Q * mcap, qcc = (size_t)Q * ccap, qb = (size_t)Q * 4;
  const size_t o_ids = k.take(qc * 4), o_vals = k.take(qc * 8), o_nw = k.take(qb), o_cf = k.take(qcc * 4), o_cs = k.take(qcc * 4), o_sc = k.take(qcc * 8), o_nc = k.take(qb),
               o_ms = k.take(qb), o_gf = k.take((size_t)Q * K * 4), o_gs = k.take((size_t)Q * K * 8), o_ng = k.take(qb), o_gst = k.take(qb), o_obj = k.take(qm * 12),
               o_img = k.take(qm * 8), o_map = k.take(qm * 4), o_X = k.take(qm * 24), o_obs = k.take(qm * 24), o_n = k.take(qb), o_nopt = k.take(qb), o_pre = k.take(qb),
               o_pnp = k.take((size_t)Q * 128), o_pmask = k.take(qm), o_pcnt = k.take(qb);
  if (k.into(c, db->r_scratch, st)) return 1;
  // map_user.cc:129-166: the vector, the query with the sharing-word filter, the scores
  if (bow_vector_queue(c, d_qfeat, d_qn, Q, cap, k.at<uint32_t>(o_ids), k.d(o_vals), k.i(o_nw), nullptr, st)) return 1;
  airfe_bowdb_filter flt;
  flt.ratio = cfg->ratio; flt.min_words = cfg->min_words; flt.d_max_index = nullptr; flt.d_exclude = nullptr; flt.exclude_words = 0;
  if (bowdb_query_queue(db, k.at<uint32_t>(o_ids), k.d(o_vals), k.i(o_nw), Q, cap, &flt, k.i(o_cf), k.i(o_cs), k.d(o_sc), ccap, k.i(o_nc), k.i(o_ms),
                        nullptr, st)) return 1;
  // :177-363: the grouping; :360-376: the matcher over the K deputies
  if (bowdb_group_queue(db, BG_MODE_RELOC, k.i(o_cf), k.d(o_sc), k.i(o_nc), Q, ccap, K, d_extra, nullptr, nullptr, k.i(o_gf), k.d(o_gs), k.i(o_ng), k.i(o_gst), st)) return 1;
  if (bowdb_match_queue(c, db, d_qfeat, d_qn, Q, cap, k.i(o_gf), K, cfg->outlier_rejection, d_best, d_idx, d_score, mcap, d_nmatch, nullptr, st)) return 1;
  // :377-390: the first gate, the winner's map points, SolvePnPWithCV
  const int refine = cfg->pose_refinement != 0;
  RelocGatherArgs g;
  g.xyz = db->xyz; g.N = N; g.cap = cap; g.qfeat = d_qfeat; g.best = d_best; g.idx = d_idx; g.nmatch = d_nmatch; g.mcap = mcap;
  g.ncand = k.i(o_nc); g.gstatus = k.i(o_gst); g.ngroups = k.i(o_ng); g.min_inlier = cfg->min_inlier; g.refine = refine;
  g.obj = k.at<float>(o_obj); g.img = k.at<float>(o_img); g.map = k.i(o_map); g.X = k.d(o_X); g.obs = k.d(o_obs);
  g.n = k.i(o_n); g.n_opt = k.i(o_nopt); g.pre = k.i(o_pre);
  launch_reloc_gather(g, Q, st);
  HIPCHK(c, hipGetLastError());
  RelocFinishArgs f;
  f.pre = g.pre; f.num = d_num; f.min_inlier = cfg->min_inlier; f.stage = d_stage; f.ok = d_ok;
  if (!refine) {
    if (pnp_queue(c, g.obj, g.img, g.n, Q, mcap, cfg->cam, d_Twc, nullptr, d_mask, mcap, g.map, d_num, st)) return 1;
    f.pnp_count = d_num; f.pnp_count_out = d_pnp_count;
  } else {
    // :392-457: the frame optimisation from the PnP pose, Tcb = identity, every constraint mono; fewer constraints than min_inlier: none are handed over
    // and the kernel returns its start pose, PnP's
    int* d_cnt = d_pnp_count ? d_pnp_count : k.i(o_pcnt);
    if (pnp_queue(c, g.obj, g.img, g.n, Q, mcap, cfg->cam, k.d(o_pnp), nullptr, k.at<uint8_t>(o_pmask), mcap, g.map, d_cnt, st)) return 1;
    if (poseopt_queue(c, g.X, g.obs, g.n_opt, Q, mcap, k.d(o_pnp), cfg->cam, nullptr, cfg->thr, d_Twc, nullptr, d_mask, mcap, g.map, d_num, -1, nullptr, st))
      return 1;
  }
  launch_reloc_finish(f, Q, st);
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(c)

/* ---- loop detection over a loaded map (include/airfe.h "Map state for loop detection", "Stored queries against their predecessors", "Loop detection
 * composite"; kernels_loopdet.hip, loopdet_core.h) -------------------------------------------------------------------------------------------------- */
int airfe_bowdb_set_poses(airfe_bowdb* db, int first_frame, int B, const double* Twc) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (!db->has_map) return fail(c, "bowdb_set_poses: no map state (airfe_bowdb_attach_map)");
  if (first_frame < 0 || B < 1 || B > db->max_frames - first_frame || !Twc) return fail(c, "bowdb_set_poses: bad argument (frames beyond max_frames)");
  std::vector<double> t((size_t)B * 3);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < 3; ++k) t[(size_t)b * 3 + k] = Twc[(size_t)b * 16 + 4 * k + 3];
  if (bowdb_rows_copy(db, db->pose, 16, first_frame, B, Twc, nullptr, hipMemcpyHostToDevice, c->stream, "bowdb_set_poses")) return 1;
  if (bowdb_rows_copy(db, db->pos, 3, first_frame, B, t.data(), nullptr, hipMemcpyHostToDevice, c->stream, "bowdb_set_poses")) return 1;
  db->has_pos = 1;
  db->has_pose = 1;
  return 0;
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_poses(airfe_bowdb* db, int first_frame, int B, double* Twc) try {
  BOWDB_ENTER(db);
  return bowdb_rows_copy(db, db->pose, 16, first_frame, B, nullptr, Twc, hipMemcpyDeviceToHost, db->c->stream, "bowdb_get_poses");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_u_right_dev(airfe_bowdb* db, int first_frame, int B, const double* d_u_right, void* stream) try {
  BOWDB_ENTER(db);
  return bowdb_rows_copy(db, db->u_right, (size_t)db->cap, first_frame, B, d_u_right, nullptr, hipMemcpyDeviceToDevice, stream_of(db->c, stream), "bowdb_set_u_right_dev");
} AIRFE_CATCH(db->c)

int airfe_bowdb_set_u_right(airfe_bowdb* db, int first_frame, int B, const double* u_right) try {
  BOWDB_ENTER(db);
  return bowdb_rows_copy(db, db->u_right, (size_t)db->cap, first_frame, B, u_right, nullptr, hipMemcpyHostToDevice, db->c->stream, "bowdb_set_u_right");
} AIRFE_CATCH(db->c)

int airfe_bowdb_get_u_right(airfe_bowdb* db, int first_frame, int B, double* u_right) try {
  BOWDB_ENTER(db);
  return bowdb_rows_copy(db, db->u_right, (size_t)db->cap, first_frame, B, nullptr, u_right, hipMemcpyDeviceToHost, db->c->stream, "bowdb_get_u_right");
} AIRFE_CATCH(db->c)

// stored frames d_qframe [Q] against their predecessors on `st`: the stored vectors gathered into d_ids / d_vals / d_nw ([Q][cap] x 2, [Q]: the caller's
// scratch), bowdb_query_kernel unchanged over the whole database, the prefix selection (the body of airfe_bowdb_query_stored_batch_dev; the loop
// detection composite queues the same code)
static int loopdet_query_queue(airfe_bowdb* db, const int32_t* d_qframe, int Q, float ratio, int min_words, int exclude_covisible, uint32_t* d_ids,
                               double* d_vals, int* d_nw, int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap, int* d_ncand,
                               int* d_max_sharing, int32_t* d_sharing, hipStream_t st) {
  const int N = db->size;
  LoopQvecArgs v;
  v.qframe = d_qframe; v.db_ids = db->ids; v.db_vals = db->vals; v.db_nw = db->nw; v.N = N; v.cap = db->cap; v.ids = d_ids; v.vals = d_vals; v.nw = d_nw;
  launch_loopdet_qvec(v, Q, st);
  LoopSelectArgs s;
  s.qframe = d_qframe; s.N = N; s.zero_tail = d_sharing ? 1 : 0; s.ratio = ratio; s.min_words = min_words;
  if (exclude_covisible) { s.row_ptr = db->cov_row; s.nbr = db->cov_nbr; s.rows = db->max_frames; }
  s.cand_frame = d_cand_frame; s.cand_sharing = d_cand_sharing; s.cand_score = d_cand_score; s.ccap = ccap; s.ncand = d_ncand; s.max_sharing = d_max_sharing;
  return query_select_queue(db, d_ids, d_vals, d_nw, Q, db->cap, d_sharing, st, "bowdb_query_stored_batch_dev", [&](double* score, int32_t* sharing) {
    s.score = score; s.sharing = sharing;
    launch_loopdet_select(s, Q, st);
  });
}

int airfe_bowdb_query_stored_batch_dev(airfe_bowdb* db, const int32_t* d_qframe, int Q, float ratio, int min_words, int exclude_covisible,
                                       int32_t* d_cand_frame, int32_t* d_cand_sharing, double* d_cand_score, int ccap, int* d_ncand, int* d_max_sharing,
                                       int32_t* d_sharing, void* stream) try {
  BOWDB_ENTER(db);
  airfe_ctx* c = db->c;
  if (Q < 1 || ccap < 1 || !d_qframe || !d_cand_frame || !d_cand_sharing || !d_cand_score || !d_ncand || !d_max_sharing)
    return fail(c, "bowdb_query_stored_batch_dev: bad argument");
  if (Q > LD_MAX_QUERIES) return fail(c, "bowdb_query_stored_batch_dev: Q > 4096");
  if (exclude_covisible && !db->has_map) return fail(c, "bowdb_query_stored_batch_dev: exclude_covisible needs the map state (airfe_bowdb_attach_map)");
  hipStream_t st = stream_of(c, stream);
  Carve k;
  const size_t qc = (size_t)Q * db->cap, o_vals = k.take(qc * 8), o_ids = k.take(qc * 4), o_nw = k.take((size_t)Q * 4);
  if (k.into(c, db->l_scratch, st)) return 1;
  return loopdet_query_queue(db, d_qframe, Q, ratio, min_words, exclude_covisible, k.at<uint32_t>(o_ids), k.d(o_vals), k.i(o_nw), d_cand_frame, d_cand_sharing,
                             d_cand_score, ccap, d_ncand, d_max_sharing, d_sharing, st);
} AIRFE_CATCH(db->c)

int airfe_loop_detect_batch_dev(airfe_ctx* c, airfe_bowdb* db, const airfe_loop_cfg* cfg, const int32_t* d_qframe, int Q, int* d_ok, int* d_stage,
                                int32_t* d_loop, double* d_Twq, double* d_Rlq, double* d_tlq, int* d_num, uint8_t* d_mask, int32_t* d_idx, float* d_score,
                                int mcap, int* d_nmatch, int* d_ncons, void* stream) try {
  AIRFE_ENTER(c);
  if (!db || db->c != c) return fail(c, "loop_detect_batch_dev: the database belongs to another context");
  if (!db->has_map) return fail(c, "loop_detect_batch_dev: no map state (airfe_bowdb_attach_map)");
  if (!db->has_pose) return fail(c, "loop_detect_batch_dev: the keyframe poses were never set (airfe_bowdb_set_poses)");
  if (!cfg || Q < 1 || mcap < 1 || !d_qframe || !d_ok || !d_stage || !d_loop || !d_Twq || !d_Rlq || !d_tlq || !d_num || !d_mask || !d_idx || !d_score ||
      !d_nmatch)
    return fail(c, "loop_detect_batch_dev: bad argument");
  if (cfg->K < 1 || cfg->K > 5) return fail(c, "loop_detect_batch_dev: cfg.K = 1..5");
  if (Q > LD_MAX_QUERIES) return fail(c, "loop_detect_batch_dev: Q > 4096");
  if (mcap > PO_MAX_POINTS) return fail(c, "loop_detect_batch_dev: mcap > 1024");
  if ((long long)Q * cfg->K > c->Pmax) return fail(c, "loop_detect_batch_dev: Q * K pairs exceed cfg.max_batch");
  const int N = db->size, ccap = std::max(N, 1), K = cfg->K, cap = db->cap;
  if (N > LD_MAX_FRAMES) return fail(c, "loop_detect_batch_dev: more than 4096 frames in the database");
  hipStream_t st = stream_of(c, stream);
  // one block, every part 256-byte aligned
  Carve k;
  const size_t qc = (size_t)Q * cap, qm = (size_t)Q * mcap, qcc = (size_t)Q * ccap, qb = (size_t)Q * 4;
  const size_t o_ids = k.take(qc * 4), o_vals = k.take(qc * 8), o_nw = k.take(qb), o_cf = k.take(qcc * 4), o_cs = k.take(qcc * 4), o_sc = k.take(qcc * 8), o_nc = k.take(qb),
               o_ms = k.take(qb), o_odom = k.take((size_t)ccap * 8), o_feat = k.take(qc * AIRFE_FEAT_DIM * 4), o_qn = k.take(qb), o_qpos = k.take((size_t)Q * 24),
               o_md = k.take((size_t)Q * 8), o_T0 = k.take((size_t)Q * 128), o_gf = k.take((size_t)Q * K * 4), o_gs = k.take((size_t)Q * K * 8), o_ng = k.take(qb),
               o_gst = k.take(qb), o_map = k.take(qm * 4), o_X = k.take(qm * 24), o_obs = k.take(qm * 24), o_n = k.take(qb), o_nopt = k.take(qb), o_pre = k.take(qb);
  if (k.into(c, db->l_scratch, st)) return 1;
  // map_refiner.cc:97-130 on the database of :88-89: frame fq against its predecessors, the covisible frames dropped
  if (loopdet_query_queue(db, d_qframe, Q, cfg->ratio, cfg->min_words, 1, k.at<uint32_t>(o_ids), k.d(o_vals), k.i(o_nw), k.i(o_cf), k.i(o_cs),
                          k.d(o_sc), ccap, k.i(o_nc), k.i(o_ms), nullptr, st)) return 1;
  // :66-81: the odometry length, once per call; what the later steps read of frame fq
  launch_loopdet_odom(db->pos, N, k.d(o_odom), st);
  LoopStateArgs s;
  s.qframe = d_qframe; s.N = N; s.cap = cap; s.db_feat = db->feat; s.db_n = db->n; s.pos = db->pos; s.pose = db->pose; s.odom = k.d(o_odom);
  s.distance_rate = cfg->distance_rate; s.qfeat = k.at<float>(o_feat); s.qn = k.i(o_qn); s.qpos = k.d(o_qpos); s.max_dist = k.d(o_md);
  s.Twc0 = k.d(o_T0);
  launch_loopdet_state(s, Q, st);
  HIPCHK(c, hipGetLastError());
  // :132-214: the grouping in loop form; :213-230: the matcher over the K deputies
  if (bowdb_group_queue(db, BG_MODE_LOOP, k.i(o_cf), k.d(o_sc), k.i(o_nc), Q, ccap, K, nullptr, k.d(o_qpos), k.d(o_md), k.i(o_gf), k.d(o_gs), k.i(o_ng), k.i(o_gst), st)) return 1;
  if (bowdb_match_queue(c, db, s.qfeat, s.qn, Q, cap, k.i(o_gf), K, cfg->outlier_rejection, d_loop, d_idx, d_score, mcap, d_nmatch, nullptr, st)) return 1;
  // :232, :241-301: the gates and the constraints
  LoopGatherArgs g;
  g.qframe = d_qframe; g.xyz = db->xyz; g.u_right = db->u_right; g.feat = db->feat; g.N = N; g.cap = cap; g.best = d_loop; g.idx = d_idx; g.nmatch = d_nmatch;
  g.mcap = mcap; g.ncand = k.i(o_nc); g.gstatus = k.i(o_gst); g.ngroups = k.i(o_ng); g.min_matches = cfg->min_matches; g.min_points = cfg->min_points;
  g.X = k.d(o_X); g.obs = k.d(o_obs); g.map = k.i(o_map); g.n = k.i(o_n); g.n_opt = k.i(o_nopt); g.pre = k.i(o_pre);
  launch_loopdet_gather(g, Q, st);
  HIPCHK(c, hipGetLastError());
  // :262, :304: the frame optimisation from the stored pose, Tcb = identity; without constraints the kernel returns its start pose
  if (poseopt_queue(c, g.X, g.obs, g.n_opt, Q, mcap, k.d(o_T0), cfg->cam, nullptr, cfg->thr, d_Twq, nullptr, d_mask, mcap, g.map, d_num, -1, nullptr, st))
    return 1;
  // :308, :327-333
  LoopFinishArgs f;
  f.pre = g.pre; f.ncons = g.n; f.num = d_num; f.min_points = cfg->min_points; f.min_inliers = cfg->min_inliers; f.best = d_loop; f.N = N;
  f.pose = db->pose; f.Twq = d_Twq; f.stage = d_stage; f.ok = d_ok; f.ncons_out = d_ncons; f.Rlq = d_Rlq; f.tlq = d_tlq;
  launch_loopdet_finish(f, Q, st);
  HIPCHK(c, hipGetLastError());
  return 0;
} AIRFE_CATCH(c)

}  // extern "C"
